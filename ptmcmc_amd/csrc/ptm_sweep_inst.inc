// ptm_sweep_inst.inc -- included by every ptm_sweep_dp*.hip with PTM_DP defined.
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

static_assert(PLAN_DENSE == KIND_DENSE && PLAN_DIAG == KIND_DIAG && PLAN_LOWER == KIND_LOWER, "ptm_sweep_plan.hpp names the kinds of ptm_kernels.hpp");

static int cu_count() {
  static const int ncu = [] {
    int dev = 0;
    hipDeviceProp_t pr;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess) return pr.multiProcessorCount;
    (void)hipGetLastError();
    return 0;
  }();
  return ncu;
}
// how many blocks of a kernel the device holds at once (0: the runtime would not say)
static int resident_blocks(const void* kernel, int threads, size_t lds) {
  int per_cu = 0;
  if (cu_count() <= 0 || hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds) != hipSuccess || per_cu <= 0) { (void)hipGetLastError(); return 0; }
  return per_cu * cu_count();
}
static hipError_t launch1(const void* kernel, int grid, int threads, size_t lds, hipStream_t st, const Dev& p) {
  void* args[] = {(void*)&p};
  return hipLaunchKernel(kernel, dim3(grid), dim3(threads), args, lds, st);
}

// ---- the builds of each family: the plan's template arguments -> the instantiation (every build there is is named here) ----
#if PTM_DP == 32
template <int MK>
static const void* mfma32_kernel_of(const SweepPlan& s) {
  static const struct { bool hist; int gen; bool ev, cpt; const void* kernel; } builds[] = {
#define PTM_B(H, G, E, C) {H, G, E, C, (const void*)sweep_mfma32_kernel<MK, H, G, E, C>}
      PTM_B(false, 0, false, false), PTM_B(true, 0, false, false), PTM_B(false, 0, false, true),   // lean (history; compacted)
      PTM_B(false, 0, true, false), PTM_B(false, 0, true, true),                                   // lean with evolving ladders
      PTM_B(false, 1, false, false), PTM_B(true, 1, false, false), PTM_B(false, 1, true, false), PTM_B(true, 1, true, false),   // the usual real-world case: uniform priors, limit bounds
      PTM_B(false, 1, false, true), PTM_B(false, 1, true, true),                                   // ... compacted
      PTM_B(false, 3, false, true), PTM_B(false, 3, true, true),                                   // ... and bounds and nothing else -- no mean, no one-dimensional moves, no mixture
      PTM_B(false, 2, false, false), PTM_B(true, 2, false, false),                                 // everything
#undef PTM_B
  };
  for (const auto& b : builds)
    if (b.hist == s.hist && b.gen == s.mgen && b.ev == s.ev && b.cpt == s.compacted) return b.kernel;
  return nullptr;
}
#endif
#if PTM_DP == 64 || PTM_DP == 128
#if PTM_DP == 64
#define PTM_MFMA_WIDE sweep_mfma64_kernel
#else
#define PTM_MFMA_WIDE sweep_mfma128_kernel
#endif
template <int MK>
static const void* mfma_wide_kernel_of(bool bnd, bool ev) {
  return bnd ? (ev ? (const void*)PTM_MFMA_WIDE<MK, true, true> : (const void*)PTM_MFMA_WIDE<MK, true, false>)
             : (ev ? (const void*)PTM_MFMA_WIDE<MK, false, true> : (const void*)PTM_MFMA_WIDE<MK, false, false>);
}
#endif
template <int KIND>
static const void* lanes_kernel_of(const SweepPlan& s) {
  if (s.family == FAM_LANES_ADA) return (const void*)sweep_lanes_ada_kernel<PTM_DP, KIND>;
  return s.gen ? (const void*)sweep_lanes_kernel<PTM_DP, KIND, true> : (const void*)sweep_lanes_kernel<PTM_DP, KIND, false>;
}
#if PTM_DP <= 32
template <int KIND>
static const void* general_kernel_of(const SweepPlan& s) {
  if (s.ada) return s.uni ? (const void*)sweep_kernel<PTM_DP, KIND, true, false, true> : (const void*)sweep_kernel<PTM_DP, KIND, false, false, true>;
  if (!s.uni) return (const void*)sweep_kernel<PTM_DP, KIND, false, false>;
  return s.simple ? (const void*)sweep_kernel<PTM_DP, KIND, true, true> : (const void*)sweep_kernel<PTM_DP, KIND, true, false>;
}
#endif

template <int KIND>
static hipError_t launch_kind(const Dev& p, const SweepPlan& s, hipStream_t st, const AdaArgs& ada) {
  const int chains = p.c_end - p.c_begin;
  (void)ada;
  switch (s.family) {
#if PTM_DP == 32
    case FAM_MFMA32: {
      const size_t lds = Mfma32Lds(nullptr, s.mgen != 0, s.compacted, chains / p.W).bytes;
      constexpr int MK = KIND == KIND_DIAG ? KIND_LOWER : KIND;   // (the plan never names a diagonal build of this family)
      const void* kf = mfma32_kernel_of<MK>(s);
      if (!kf) return hipErrorNotSupported;
      // a persistent grid of the resident blocks for the lean and the compacted builds, one block per 256-chain tile for the others
      // (PTM_MFMA_GEN_PERSIST); PTM_PERSIST=n in the environment: n blocks per CU, 0: one block per tile for all (A/B measurements)
      static const int persist = [] { const char* v = getenv("PTM_PERSIST"); return v && *v ? atoi(v) : -1; }();
      int grid = (chains + 255) / 256;
      if (persist != 0 && (s.mgen == 0 || s.compacted || PTM_MFMA_GEN_PERSIST)) {
        const int ncu = cu_count() > 0 ? cu_count() : 256;
        int g = persist > 0 ? ncu * persist : resident_blocks(kf, 256, lds);
        if (g <= 0) g = ncu * 2;
        if (g < grid) grid = g;
      }
      return launch1(kf, grid, 256, lds, st, p);
    }
#endif
#if PTM_DP == 64 || PTM_DP == 128
    case FAM_MFMA64:
    case FAM_MFMA128: {
      // (the 128-D kernel: 97 KB of LDS, one block per CU)
      constexpr int MK = KIND == KIND_DIAG ? KIND_LOWER : KIND;   // (the plan never names a diagonal build of this family)
#if PTM_DP == 64
      constexpr int threads = 256;
      const size_t lds = Mfma64Lds(nullptr).bytes;
#else
      constexpr int threads = M128_THREADS;
      const size_t lds = Mfma128Lds(nullptr).bytes;
#endif
      static int resident = 0;   // (per factor kind; of the build with the most registers: the same grid for all four)
      if (!resident) {
#if PTM_DP == 128
        for (int k = 0; k < 4; ++k)
          if (hipFuncSetAttribute(mfma_wide_kernel_of<MK>(k & 2, k & 1), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return hipGetLastError();
#endif
        resident = resident_blocks(mfma_wide_kernel_of<MK>(true, true), threads, lds);
        if (!resident) resident = PTM_DP == 64 ? 512 : 256;
      }
      const int ntiles = (chains + threads - 1) / threads;
      return launch1(mfma_wide_kernel_of<MK>(s.bnd, s.ev), resident < ntiles ? resident : ntiles, threads, lds, st, p);
    }
#endif
    case FAM_LANES:
    case FAM_LANES_ADA: {
      constexpr int CPW = PTM_DP > 64 ? 1 : 64 / PTM_DP;   // chains per wave
      const size_t lds = (size_t)lanes_lds_doubles<PTM_DP>(4) * sizeof(double);
      const void* kf = lanes_kernel_of<KIND>(s);
      if (lds > 64 * 1024) {   // (65..128 dimensions: the packed precision matrix alone is 66 KB)
        hipError_t rc = hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (rc != hipSuccess) return rc;
      }
      void* args[] = {(void*)&p, (void*)&ada};
      return hipLaunchKernel(kf, dim3((chains + 4 * CPW - 1) / (4 * CPW)), dim3(256), args, lds, st);
    }
#if PTM_DP <= 32
    case FAM_GENERAL: {
      const size_t lds = GeneralLds(nullptr, s.uni && KIND != KIND_DIAG, p.prop_stride).bytes;
      const AdaArgs none = AdaArgs();
      void* args[] = {(void*)&p, (void*)(s.ada ? &ada : &none)};
      return hipLaunchKernel(general_kernel_of<KIND>(s), dim3((chains + 255) / 256), dim3(256), args, lds, st);
    }
#endif
    default: return hipErrorNotSupported;
  }
}

static hipError_t launch_sweep(const Dev& p, const SweepPlan& s, hipStream_t st, const AdaArgs& ada) {
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
static hipError_t launch_fused(const Dev& p, const Decide& d, bool diag, int nsteps, int* swap_log_base, int log_head, size_t decide_lds, hipStream_t st) {
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
static size_t ladder_lds(int Nt, int ms, bool ev) {
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
static int ladder_blocks(bool diag, int fl, size_t lds) {
  const void* kf = ladder_kernel_of(diag, fl);
  if (lds > 64 * 1024 && hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return resident_blocks(kf, LADDER_THREADS, lds);
}
static hipError_t launch_ladder(const Dev& p, const LadderArgs& a, bool diag, int fl, int grid, size_t lds, hipStream_t st) {
  void* args[] = {(void*)&p, (void*)&a};
  return hipLaunchKernel(ladder_kernel_of(diag, fl), dim3(grid), dim3(LADDER_THREADS), args, lds, st);
}
#endif

static hipError_t launch_eval(const Dev& p, int n, double* x, int* valid, double* lp, double* ll, int eval_like, hipStream_t st) {
  hipLaunchKernelGGL((evaluate_kernel<PTM_DP>), dim3((n + 255) / 256), dim3(256), 0, st, p, n, x, valid, lp, ll, eval_like);
  return hipGetLastError();
}

static hipError_t launch_init(const Dev& p, double* x, double* ll, double* lp, int* fail, long long cb_attempt, unsigned char* pending, hipStream_t st) {
  hipLaunchKernelGGL((init_prior_kernel<PTM_DP>), dim3((p.Nc + 255) / 256), dim3(256), 0, st, p, x, ll, lp, fail, cb_attempt, pending);
  return hipGetLastError();
}

// this dimension's entry of the launch table (ptm_launch.hpp); host code only
#if !defined(__HIP_DEVICE_COMPILE__)
extern const DpLaunch PTM_CAT(dp_launch_, PTM_DP) = {
    launch_sweep, launch_eval, launch_init,
#if PTM_DP <= 16
    launch_fused,
#else
    nullptr,
#endif
#if PTM_DP <= 32
    ladder_lds, ladder_blocks, launch_ladder,
#else
    nullptr, nullptr, nullptr,
#endif
};
#endif

}  // namespace ptm
