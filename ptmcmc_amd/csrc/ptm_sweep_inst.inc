// ptm_sweep_inst.inc -- included by ptm_sweep_dp{4,8,16,32}.hip with PTM_DP defined.
#include <cstdlib>

#include "ptm_launch.hpp"
#if PTM_DP == 32
#include "ptm_mfma_kernel.hpp"
#endif
#if PTM_DP == 64
#include "ptm_mfma64_kernel.hpp"
#endif
#if PTM_DP == 128
#include "ptm_mfma128_kernel.hpp"
#endif
#include "ptm_lanes_kernel.hpp"
#if PTM_DP <= 16
#include "ptm_fused_kernel.hpp"
#endif
#if PTM_DP <= 32
#include "ptm_ladder_kernel.hpp"
#endif

#define PTM_CAT2(a, b) a##b
#define PTM_CAT(a, b) PTM_CAT2(a, b)

namespace ptm {

// PTM_FORCE_VALU=1 in the environment keeps the VALU kernel on the MFMA kernel's workload (A/B measurements, tests)
#if PTM_DP == 32
// resident blocks of the MFMA kernel per CU for its persistent grid (ptm_mfma_kernel.hpp); PTM_PERSIST=0 in the environment
// launches one block per 256-chain tile instead (A/B measurements)
static int mfma_grid_blocks(const void* kernel, size_t lds, int ntiles, bool general) {
  static const int persist = [] { const char* s = getenv("PTM_PERSIST"); return s && *s ? atoi(s) : -1; }();
  if (persist == 0 || (general && !PTM_MFMA_GEN_PERSIST)) return ntiles;
  static int ncu = 0;
  if (!ncu) {
    int dev = 0;
    hipDeviceProp_t pr;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess) ncu = pr.multiProcessorCount;
    if (ncu <= 0) ncu = 256;
  }
  int per_cu = persist > 0 ? persist : 0;
  if (per_cu == 0 && hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, lds) != hipSuccess) per_cu = 0;
  if (per_cu <= 0) per_cu = 2;
  const int g = ncu * per_cu;
  return g < ntiles ? g : ntiles;
}
#endif

static bool force_valu_path() {
  static const bool v = [] { const char* s = getenv("PTM_FORCE_VALU"); return s && *s && *s != '0'; }();
  return v;
}

template <int KIND>
static hipError_t launch_kind(const Dev& p, SweepSel s, hipStream_t st, const AdaArgs& ada) {
  const dim3 grid((p.c_end - p.c_begin + 255) / 256), block(256);
  // UNI kernels stage one copy of the rung's factor per wave in LDS (4 waves per block)
  // plus the 20 KB of Box-Muller tables every variant stages
  const size_t tab = BM_TABLE_DOUBLES * sizeof(double);
  const size_t lds = tab + ((s.uni && KIND != KIND_DIAG) ? (size_t)4 * p.prop_stride * sizeof(double) : 0);
#if PTM_DP == 32
  if (s.uni && p.mode == 0 && !s.callback && !s.host_prop && !s.de && !s.ada && !force_valu_path()) {
    constexpr int MK = KIND == KIND_DIAG ? KIND_LOWER : KIND;   // a diagonal factor is a (very sparse) Cholesky factor
    // the BASELINE workload: both matrix products on the f64 matrix cores (ptm_mfma_kernel.hpp)
    // LDS: tables | P2 tiles | box | 4 x 128 reduction slots | (general: 6 x 32 doubles + 3 x 32 ints + 4 x 128 slots)
    const size_t mlds_lean = (BM_TABLE_DOUBLES + 12 * 64 + 64 + 4 * 128) * sizeof(double);
    const size_t mlds = (s.simple || s.lean_ev) ? mlds_lean : mlds_lean + (6 * 32 + 48 + 4 * 128 + 64) * sizeof(double);
    const bool hist = p.hist.rungs != 0 || p.map.rungs != 0;   // the build that carries history / MAP code
    const int ntiles = (p.c_end - p.c_begin + 255) / 256;
#define PTM_LAUNCH_MFMA(...)                                                                             \
    do {                                                                                                 \
      const void* kf = (const void*)(__VA_ARGS__);                                                       \
      hipLaunchKernelGGL((__VA_ARGS__), dim3(mfma_grid_blocks(kf, mlds, ntiles, !s.simple)), block, mlds, st, p);   \
    } while (0)
    if (s.simple && !hist && p.cidx) {   // compacted: the moving chains only (the engine ran partition_kernel)
      const size_t mlds0 = mlds;
      const size_t mlds = mlds0 + ((size_t)(p.c_end - p.c_begin) / p.W + 260) * sizeof(int);
      PTM_LAUNCH_MFMA(sweep_mfma32_kernel<MK, false, 0, false, true>);
    } else if (s.simple) {
      if (hist) PTM_LAUNCH_MFMA(sweep_mfma32_kernel<MK, true, 0>);
      else PTM_LAUNCH_MFMA(sweep_mfma32_kernel<MK, false, 0>);
    } else if (s.lean_ev) {   // the plain workload with evolving ladders: the lean build reading per-chain temperatures
      const void* kf = p.cidx ? (const void*)sweep_mfma32_kernel<MK, false, 0, true, true> : (const void*)sweep_mfma32_kernel<MK, false, 0, true, false>;
      const size_t mlds_ev = mlds + (p.cidx ? ((size_t)(p.c_end - p.c_begin) / p.W + 260) * sizeof(int) : 0);
      const dim3 grid(mfma_grid_blocks(kf, mlds_ev, ntiles, false));
      if (p.cidx) hipLaunchKernelGGL((sweep_mfma32_kernel<MK, false, 0, true, true>), grid, block, mlds_ev, st, p);
      else hipLaunchKernelGGL((sweep_mfma32_kernel<MK, false, 0, true, false>), grid, block, mlds_ev, st, p);
    } else if (p.all_uniform && (!p.has_bounds || p.bounds_box) && !hist && p.cidx) {   // ... compacted (no history)
      const size_t mlds0 = mlds;
      const size_t mlds = mlds0 + ((size_t)(p.c_end - p.c_begin) / p.W + 260) * sizeof(int);
      const bool general = false;   // (a persistent grid, like the lean build's)
#define PTM_LAUNCH_MFMA_P(...)                                                                           \
      do {                                                                                               \
        const void* kf = (const void*)(__VA_ARGS__);                                                     \
        hipLaunchKernelGGL((__VA_ARGS__), dim3(mfma_grid_blocks(kf, mlds, ntiles, general)), block, mlds, st, p);   \
      } while (0)
      // (bounds and nothing else -- no mean, no one-dimensional moves, no mixture: the build that carries none of them, GEN 3)
      const bool lite = !p.has_mean && !p.any_oned && p.mix_K == 0;
      if (lite && p.betaC) PTM_LAUNCH_MFMA_P(sweep_mfma32_kernel<MK, false, 3, true, true>);
      else if (lite) PTM_LAUNCH_MFMA_P(sweep_mfma32_kernel<MK, false, 3, false, true>);
      else if (p.betaC) PTM_LAUNCH_MFMA_P(sweep_mfma32_kernel<MK, false, 1, true, true>);
      else PTM_LAUNCH_MFMA_P(sweep_mfma32_kernel<MK, false, 1, false, true>);
#undef PTM_LAUNCH_MFMA_P
    } else if (p.all_uniform && (!p.has_bounds || p.bounds_box) && !p.betaC) {   // the usual real-world case: uniform priors, limit bounds
      if (hist) PTM_LAUNCH_MFMA(sweep_mfma32_kernel<MK, true, 1>);
      else PTM_LAUNCH_MFMA(sweep_mfma32_kernel<MK, false, 1>);
    } else if (p.all_uniform && (!p.has_bounds || p.bounds_box)) {                // ... with evolving ladders
      if (hist) PTM_LAUNCH_MFMA(sweep_mfma32_kernel<MK, true, 1, true>);
      else PTM_LAUNCH_MFMA(sweep_mfma32_kernel<MK, false, 1, true>);
    } else {
      if (hist) PTM_LAUNCH_MFMA(sweep_mfma32_kernel<MK, true, 2>);
      else PTM_LAUNCH_MFMA(sweep_mfma32_kernel<MK, false, 2>);
    }
#undef PTM_LAUNCH_MFMA
    return hipGetLastError();
  }
#endif
#if PTM_DP == 64
  // 33..64 dimensions, whole waves per rung, the plain workload without history: both products on the f64 matrix cores
  // (ptm_mfma64_kernel.hpp); everything else at these dimensions keeps the lanes kernel
  // (the plain workload, or open / `limit` bounds and / or evolving ladders on top of it: template flags BND, EV)
  if (s.uni && p.all_uniform && (!p.has_bounds || p.bounds_box) && !p.has_mean && !p.any_oned && p.mix_K == 0 && !s.ada && p.mode == 0 && !s.callback && !s.host_prop &&
      !p.hist.rungs && !p.map.rungs && !force_valu_path()) {
    constexpr int MK = KIND == KIND_DIAG ? KIND_LOWER : KIND;   // a diagonal factor is a (very sparse) Cholesky factor
    const size_t mlds = (size_t)m64_lds_doubles() * sizeof(double);
    const bool bnd = p.has_bounds != 0, ev = p.betaC != nullptr;
    const void* kf = bnd ? (ev ? (const void*)sweep_mfma64_kernel<MK, true, true> : (const void*)sweep_mfma64_kernel<MK, true, false>)
                         : (ev ? (const void*)sweep_mfma64_kernel<MK, false, true> : (const void*)sweep_mfma64_kernel<MK, false, false>);
    const int ntiles = (p.c_end - p.c_begin + 255) / 256;
    static int resident = 0;
    if (!resident) {
      int dev = 0, per_cu = 0;
      hipDeviceProp_t pr;
      if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess &&
          hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)sweep_mfma64_kernel<MK, true, true>, 256, mlds) == hipSuccess && per_cu > 0)
        resident = per_cu * pr.multiProcessorCount;   // (the build with the most registers: the same grid for all four)
      else { (void)hipGetLastError(); resident = 512; }
    }
    void* args[] = {(void*)&p};
    return hipLaunchKernel(kf, dim3(resident < ntiles ? resident : ntiles), block, args, mlds, st);
  }
#endif
#if PTM_DP == 128
  // 65..128 dimensions, whole waves per rung, the plain workload without history: both products on the f64 matrix cores
  // (ptm_mfma128_kernel.hpp: 97 KB of LDS, one block per CU); everything else at these dimensions keeps the lanes kernel
  // (the plain workload, or open / `limit` bounds and / or evolving ladders on top of it: template flags BND, EV)
  if (s.uni && p.all_uniform && (!p.has_bounds || p.bounds_box) && !p.has_mean && !p.any_oned && p.mix_K == 0 && !s.ada && p.mode == 0 && !s.callback && !s.host_prop &&
      !p.hist.rungs && !p.map.rungs && !force_valu_path()) {
    constexpr int MK = KIND == KIND_DIAG ? KIND_LOWER : KIND;   // a diagonal factor is a (very sparse) Cholesky factor
    const size_t mlds = (size_t)m128_lds_doubles() * sizeof(double);
    const bool bnd = p.has_bounds != 0, ev = p.betaC != nullptr;
    const void* kf = bnd ? (ev ? (const void*)sweep_mfma128_kernel<MK, true, true> : (const void*)sweep_mfma128_kernel<MK, true, false>)
                         : (ev ? (const void*)sweep_mfma128_kernel<MK, false, true> : (const void*)sweep_mfma128_kernel<MK, false, false>);
    const int ntiles = (p.c_end - p.c_begin + M128_THREADS - 1) / M128_THREADS;
    static int resident = 0;
    if (!resident) {
      int dev = 0, per_cu = 0;
      hipDeviceProp_t pr;
      const void* all4[] = {(const void*)sweep_mfma128_kernel<MK, false, false>, (const void*)sweep_mfma128_kernel<MK, false, true>,
                            (const void*)sweep_mfma128_kernel<MK, true, false>, (const void*)sweep_mfma128_kernel<MK, true, true>};
      for (const void* f : all4)
        if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mlds) != hipSuccess) return hipGetLastError();
      if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess &&
          hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, all4[3], M128_THREADS, mlds) == hipSuccess && per_cu > 0)
        resident = per_cu * pr.multiProcessorCount;
      else { (void)hipGetLastError(); resident = 256; }
    }
    void* args[] = {(void*)&p};
    return hipLaunchKernel(kf, dim3(resident < ntiles ? resident : ntiles), dim3(M128_THREADS), args, mlds, st);
  }
#endif
  // (33..128 dimensions: the lanes kernel serves small populations and the general workloads)
  // (the host-callback passes -- mode 1 / 2 -- are in its general build; up to 8 dimensions a chain is little work for
  //  one lane, and the lanes kernel is the choice of the latency regime only)
  constexpr long long LANES_MAX = PTM_DP >= 16 ? PTM_LANES_MAX : 4096ll * PTM_DP;
  // (differential evolution keeps a population with whole waves per rung off the matrix cores: from 9 dimensions on its moderate sizes
  //  are better off with a lane per dimension than with a lane walking a chain)
  //  (measured, tools/de_probe_walkers.sh, us per step lanes / lane-per-chain: 12 dimensions x 4096 chains 40 / 57, x 16384 50 / 62,
  //   x 65536 96 / 75; 32 dimensions x 8192 chains 49 / 131)
  constexpr long long LANES_MAX_DE = PTM_DP >= 32 ? (1ll << 21) : (1ll << 19);
  const long long lanes_wanted = (long long)(p.c_end - p.c_begin) * PTM_DP;
  if (PTM_DP >= 64 || s.host_prop || (!force_valu_path() && ((!s.uni && lanes_wanted <= LANES_MAX) || (s.uni && s.de && PTM_DP >= 16 && lanes_wanted <= LANES_MAX_DE)))) {
    // small populations (fewer than 64 walkers per rung): a lane per dimension instead of a lane per chain -- a sixteenth
    // of the latency, twice the lane-work per chain: the better trade until the chip is full of waves
    constexpr int CPW = PTM_DP > 64 ? 1 : 64 / PTM_DP;
    const dim3 lgrid((p.c_end - p.c_begin + 4 * CPW - 1) / (4 * CPW));
    const size_t llds = (size_t)lanes_lds_doubles<PTM_DP>(4) * sizeof(double);
    if (llds > 64 * 1024) {   // (65..128 dimensions: the packed precision matrix alone is 66 KB)
      hipError_t rc = hipFuncSetAttribute(s.ada ? (const void*)sweep_lanes_ada_kernel<PTM_DP, KIND>
                                                : s.plain ? (const void*)sweep_lanes_kernel<PTM_DP, KIND, false> : (const void*)sweep_lanes_kernel<PTM_DP, KIND, true>,
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)llds);
      if (rc != hipSuccess) return rc;
    }
    if (s.ada) hipLaunchKernelGGL((sweep_lanes_ada_kernel<PTM_DP, KIND>), lgrid, block, llds, st, p, ada);
    else if (s.plain) hipLaunchKernelGGL((sweep_lanes_kernel<PTM_DP, KIND, false>), lgrid, block, llds, st, p);
    else hipLaunchKernelGGL((sweep_lanes_kernel<PTM_DP, KIND, true>), lgrid, block, llds, st, p);
    return hipGetLastError();
  }
#if PTM_DP <= 32
  if (s.ada && s.uni) hipLaunchKernelGGL((sweep_kernel<PTM_DP, KIND, true, false, true>), grid, block, lds, st, p, ada);
  else if (s.ada) hipLaunchKernelGGL((sweep_kernel<PTM_DP, KIND, false, false, true>), grid, block, tab, st, p, ada);
  else if (s.uni && s.simple) hipLaunchKernelGGL((sweep_kernel<PTM_DP, KIND, true, true>), grid, block, lds, st, p, AdaArgs());
  else if (s.uni) hipLaunchKernelGGL((sweep_kernel<PTM_DP, KIND, true, false>), grid, block, lds, st, p, AdaArgs());
  else hipLaunchKernelGGL((sweep_kernel<PTM_DP, KIND, false, false>), grid, block, tab, st, p, AdaArgs());
  return hipGetLastError();
#else
  (void)grid; (void)lds; (void)tab;
  return hipErrorNotSupported;
#endif
}

hipError_t PTM_CAT(launch_sweep_, PTM_DP)(const Dev& p, SweepSel s, hipStream_t st, const AdaArgs& ada) {
  switch (s.kind) {
    case KIND_DIAG: return launch_kind<KIND_DIAG>(p, s, st, ada);
    case KIND_LOWER: return launch_kind<KIND_LOWER>(p, s, st, ada);
    default: return launch_kind<KIND_DENSE>(p, s, st, ada);
  }
}

#if PTM_DP <= 16
template <int KIND, int T>
static hipError_t launch_fused_kt(const Dev& p, const Decide& d, int nsteps, int* swap_log_base, int log_head, size_t decide_lds, hipStream_t st) {
  const size_t lds = (size_t)((lanes_lds_doubles<PTM_DP>(T / 64) + 1) & ~1) * sizeof(double) + decide_lds;
  if (lds > 64 * 1024) {
    hipError_t rc = hipFuncSetAttribute((const void*)ladder_steps_kernel<PTM_DP, KIND, T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (rc != hipSuccess) return rc;
  }
  hipLaunchKernelGGL((ladder_steps_kernel<PTM_DP, KIND, T>), dim3(p.W), dim3(T), lds, st, p, d, nsteps, swap_log_base, log_head);
  return hipGetLastError();
}
hipError_t PTM_CAT(launch_fused_, PTM_DP)(const Dev& p, const Decide& d, bool diag, int nsteps, int* swap_log_base, int log_head, size_t decide_lds,
                                          hipStream_t st) {
  const int lanes = p.Nt * PTM_DP;
#define PTM_FUSED_T(T)                                                                                                        \
  return diag ? launch_fused_kt<KIND_DIAG, T>(p, d, nsteps, swap_log_base, log_head, decide_lds, st)                            \
              : launch_fused_kt<KIND_DENSE, T>(p, d, nsteps, swap_log_base, log_head, decide_lds, st)
  if (lanes <= 64) { PTM_FUSED_T(64); }
  if (lanes <= 256) { PTM_FUSED_T(256); }
#undef PTM_FUSED_T
  // (a 1024-thread form was built and dropped: sixteen waves leave 128 registers per lane, the two bodies plus what the
  //  optimiser hoists out of the step loop spill ~100 of them, and the result was no faster than the two launches:
  //  BASELINE configs[1], 64 rungs x 16 dimensions, 15.2 against 15.0 us per step)
  return hipErrorNotSupported;
}
#endif

#if PTM_DP <= 32
// the persistent ladder kernel (ptm_ladder_kernel.hpp): DENSE serves Cholesky factors too (a lane reads its whole row)
size_t PTM_CAT(ladder_lds_, PTM_DP)(int Nt, int ms, bool ev) {
  return (size_t)((lanes_lds_doubles<PTM_DP>(4) + 1) & ~1) * sizeof(double) + ladder_decide_lds_bytes(Nt, ms) + ladder_window_lds_bytes(PTM_DP) + ladder_psq_lds_bytes(PTM_DP) + 16 +
         (ev ? ladder_ev_lds_bytes(Nt, ms) : 0);
}
// the kernel's builds: FL bit 0 = one-dimensional moves + scale mixtures, bit 1 = history ring + MAP tracking, bit 2 = evolving ladders
// (built plain, 4, and with everything, 7: the reference sampler's defaults), bit 3 = differential evolution from the history ring (11, 15), bit 4 = any boundary / any per-dimension prior (19, 23, 27, 31: with the recipe's and the history's code, whether or not the engine uses them)
static const void* ladder_kernel_of(bool diag, int fl) {
#define PTM_LK(K, F) (const void*)ladder_persistent_kernel<PTM_DP, K, F>
  switch (fl & 31) {
    case 19: return diag ? PTM_LK(KIND_DIAG, 19) : PTM_LK(KIND_DENSE, 19);
    case 23: return diag ? PTM_LK(KIND_DIAG, 23) : PTM_LK(KIND_DENSE, 23);
    case 27: return diag ? PTM_LK(KIND_DIAG, 27) : PTM_LK(KIND_DENSE, 27);
    case 31: return diag ? PTM_LK(KIND_DIAG, 31) : PTM_LK(KIND_DENSE, 31);
    case 11: return diag ? PTM_LK(KIND_DIAG, 11) : PTM_LK(KIND_DENSE, 11);
    case 15: return diag ? PTM_LK(KIND_DIAG, 15) : PTM_LK(KIND_DENSE, 15);
    case 0: return diag ? PTM_LK(KIND_DIAG, 0) : PTM_LK(KIND_DENSE, 0);
    case 1: return diag ? PTM_LK(KIND_DIAG, 1) : PTM_LK(KIND_DENSE, 1);
    case 2: return diag ? PTM_LK(KIND_DIAG, 2) : PTM_LK(KIND_DENSE, 2);
    case 3: return diag ? PTM_LK(KIND_DIAG, 3) : PTM_LK(KIND_DENSE, 3);
    case 4: return diag ? PTM_LK(KIND_DIAG, 4) : PTM_LK(KIND_DENSE, 4);
    default: return diag ? PTM_LK(KIND_DIAG, 7) : PTM_LK(KIND_DENSE, 7);
  }
#undef PTM_LK
}
// how many workgroups of that build the device holds at once (the dynamic-LDS attribute is set on THIS build: asked per build)
int PTM_CAT(ladder_blocks_, PTM_DP)(bool diag, int fl, size_t lds) {
  const void* kf = ladder_kernel_of(diag, fl);
  if (lds > 64 * 1024 && hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) { (void)hipGetLastError(); return 0; }
  int dev = 0, per_cu = 0;
  hipDeviceProp_t pr;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&pr, dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kf, LADDER_THREADS, lds) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return per_cu > 0 ? per_cu * pr.multiProcessorCount : 0;
}
hipError_t PTM_CAT(launch_ladder_, PTM_DP)(const Dev& p, const LadderArgs& a, bool diag, int fl, int grid, size_t lds, hipStream_t st) {
  void* args[] = {(void*)&p, (void*)&a};
  return hipLaunchKernel(ladder_kernel_of(diag, fl), dim3(grid), dim3(LADDER_THREADS), args, lds, st);
}
#endif

hipError_t PTM_CAT(launch_eval_, PTM_DP)(const Dev& p, int n, double* x, int* valid, double* lp, double* ll, int eval_like,
                                         hipStream_t st) {
  hipLaunchKernelGGL((evaluate_kernel<PTM_DP>), dim3((n + 255) / 256), dim3(256), 0, st, p, n, x, valid, lp, ll, eval_like);
  return hipGetLastError();
}

hipError_t PTM_CAT(launch_init_, PTM_DP)(const Dev& p, double* x, double* ll, double* lp, int* fail, long long cb_attempt,
                                         unsigned char* pending, hipStream_t st) {
  hipLaunchKernelGGL((init_prior_kernel<PTM_DP>), dim3((p.Nc + 255) / 256), dim3(256), 0, st, p, x, ll, lp, fail, cb_attempt, pending);
  return hipGetLastError();
}

}  // namespace ptm
