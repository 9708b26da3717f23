// ptm_launch.hpp -- host-side launch entry points of the per-dimension translation units.
// The fused sweep kernel is instantiated for DP in {4,8,16,32,64,128,256,512,1024}; each DP lives in its own .hip file so the
// (large, fully unrolled) kernels compile in parallel.
#pragma once
#include <hip/hip_runtime.h>

#include "ptm_decide.hpp"
#include "ptm_kernels.hpp"
#include "ptm_ladder_args.hpp"
#include "ptm_sweep_plan.hpp"

namespace ptm {
// One padded dimension's launches (defined by its translation unit through ptm_sweep_inst.inc); an entry is null where the dimension
// does not build the path.
struct DpLaunch {
  // one MH sweep on the build the plan names (ptm_sweep_plan.hpp)
  hipError_t (*sweep)(const Dev& p, const SweepPlan& s, hipStream_t st, const AdaArgs& ada);
  hipError_t (*eval)(const Dev& p, int n, double* x, int* valid, double* lp, double* ll, int eval_like, hipStream_t st);
  hipError_t (*init)(const Dev& p, double* x, double* ll, double* lp, int* fail, long long cb_attempt, unsigned char* pending, hipStream_t st);
  // small ladders: nsteps whole PT steps per launch, one block per walker-ladder (ptm_fused_kernel.hpp; built for DP <= 16)
  hipError_t (*fused)(const Dev& p, const Decide& d, bool diag, int nsteps, int* swap_log_base, int log_head, size_t decide_lds, hipStream_t st);
  // long ladders of few walkers: many PT steps per launch on a grid of resident workgroups (ptm_ladder_kernel.hpp; DP <= 32).
  // ladder_blocks: how many of its workgroups the device holds at once (0: the kernel cannot run); launch_ladder: the launch
  size_t (*ladder_lds)(int Nt, int ms, bool ev);
  int (*ladder_blocks)(bool diag, int fl, size_t lds);
  hipError_t (*launch_ladder)(const Dev& p, const LadderArgs& a, bool diag, int fl, int grid, size_t lds, hipStream_t st);
};
extern const DpLaunch dp_launch_4, dp_launch_8, dp_launch_16, dp_launch_32, dp_launch_64, dp_launch_128, dp_launch_256, dp_launch_512, dp_launch_1024;
const DpLaunch* dp_launch(int DP);   // (null: no such padded dimension)
}  // namespace ptm
