// The facade's proposal_tester (ptmcmc_gpu.hh) on three proposals: a native Gaussian, a correct symmetric device_proposal (a HIP
// kernel) and a wrong one, the contraction y = c + 0.9 (x - c) with a claimed log-Hastings ratio of 0.  Three dimensions, one
// wrapped, one cut by a `limit` bound.  Prints the tester's lines, then one line
//   RESULT accept=<rate of the last cycle> moved=<0|1> alt_fkl=<value> fkl_redraw_max=<value> kl=<PASS|FAIL> fkl=<PASS|FAIL>
// Compiled as HIP (-x hip).  Checked by tests/test_gpu_proposal_test.py.
//   usage: proposal_test native|device|contraction|native_err|host|host_err|seam [outpath]      (host*: 256 samples through the host-proposal step;
//                                                     seam: the wrapped dimension's target 1.25 sigma from its seam -- refused)
//          proposal_test sampler <outbase> [--prop_test_index=...]     the sampler of examples/example_sampler.cc, 300 steps, the test at 512 samples x 5 cycles x 2 redraws
//          proposal_test sampler_wrap <outbase> [...]   the same with dimension a wrapped on [0, 2 pi) and its prior [0.05, 0.35], beside the seam; 2048 x 10 x 4
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ptmcmc_gpu.hh"
using namespace ptmgpu;

static const int D = 3, NSAMP = 2048, NTRY = 4;
static const double NCYC = 10;
__constant__ double c_centre[D] = {3.0, 0.0, -2.0};
__constant__ double c_scale[D] = {0.7 * 0.4, 0.7 * 0.5, 0.7 * 2.0};
static const double CENTRE[D] = {3.0, 0.0, -2.0}, SIGMA[D] = {0.4, 0.5, 2.0};

__host__ __device__ inline uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ inline double uniform_of(uint64_t key) { return ((double)(mix64(key) >> 11) + 0.5) * (1.0 / 9007199254740992.0); }

// x' = x + scale * z, z standard normal from a counter hash of (step, replica, dimension): symmetric, log-Hastings 0 (the preset)
__global__ __launch_bounds__(256) void symmetric_kernel(int n, const double* __restrict__ X, const int32_t* __restrict__ walker, uint64_t step,
                                                        double* __restrict__ Xp) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n * D) return;
  const int row = k / D, d = k - row * D;
  const uint64_t key = (step * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)walker[row] << 20) ^ (uint64_t)(d * 2);
  const double z = sqrt(-2.0 * log(uniform_of(key))) * cos(6.283185307179586 * uniform_of(key + 1));
  Xp[k] = X[k] + c_scale[d] * z;
}
// y = c + 0.9 (x - c): always uphill, so always accepted with the ratio it claims (0, the preset) -- and not invariant
__global__ __launch_bounds__(256) void contraction_kernel(int n, const double* __restrict__ X, double* __restrict__ Xp) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n * D) return;
  const int d = k % D;
  Xp[k] = c_centre[d] + 0.9 * (X[k] - c_centre[d]);
}

class kernel_proposal : public device_proposal {
  bool contraction;

 public:
  explicit kernel_proposal(bool contraction) : contraction(contraction) {}
  void draw_device(void* stream, int n_rows, int dim, const double* X_cur_dev, const int32_t*, const int32_t* walker_dev, const int32_t*, uint64_t step,
                   double* X_prop_dev, double*, int32_t*, int32_t*) override {
    if (dim != D || n_rows < 1) return;
    const dim3 grid((n_rows * D + 255) / 256);
    if (contraction) hipLaunchKernelGGL(contraction_kernel, grid, dim3(256), 0, (hipStream_t)stream, n_rows, X_cur_dev, X_prop_dev);
    else hipLaunchKernelGGL(symmetric_kernel, grid, dim3(256), 0, (hipStream_t)stream, n_rows, X_cur_dev, walker_dev, step, X_prop_dev);
  }
  state draw(state& s, chain* caller) override {   // (the host form, for the host-proposal step: the same kinds of move)
    std::vector<double> x = s.get_params_vector();
    for (int d = 0; d < D; d++) {
      if (contraction) x[d] = CENTRE[d] + 0.9 * (x[d] - CENTRE[d]);
      else x[d] += 0.7 * SIGMA[d] * detail::normal_from(*caller->getPRNG());
    }
    log_hastings = 0;
    return state(s.getSpace(), x);
  }
  proposal_distribution* clone() const override { return new kernel_proposal(*this); }
  std::string show() override { return contraction ? "Contraction()" : "SymmetricKernel()"; }
};

// a host-side proposal: the same symmetric step, drawn by draw() only
class host_symmetric : public proposal_distribution {
 public:
  state draw(state& s, chain* caller) override {
    std::vector<double> x = s.get_params_vector();
    for (int d = 0; d < D; d++) x[d] += 0.7 * SIGMA[d] * detail::normal_from(*caller->getPRNG());
    log_hastings = 0;
    return state(s.getSpace(), x);
  }
  proposal_distribution* clone() const override { return new host_symmetric(*this); }
  std::string show() override { return "HostSymmetric()"; }
};

// examples/example_sampler.cc with a short run; the flags after the outbase are the sampler's
static int sampler_run(int argc, char** argv, bool wrap) {
  if (argc < 3) return 2;
  std::vector<double> P = {2.0, 0.6, 0.0, 0.6, 1.0, -0.3, 0.0, -0.3, 1.5};
  stateSpace space(D);
  space.set_names(std::vector<std::string>{"a", "b", "c"});
  if (wrap) space.set_bound(0, boundary(boundary::wrap, boundary::wrap, 0.0, 2 * M_PI));
  gaussian_likelihood like(P, 0.0);
  std::vector<double> centers(D, 0.0), scales(D, 20.0);
  if (wrap) { centers[0] = 0.2; scales[0] = 0.15; }
  like.basic_setup(&space, std::vector<std::string>(D, "uni"), centers, scales);
  std::vector<proposal_distribution*> gset;
  std::vector<double> gshares;
  double fac = std::pow(2.0 / 4.0, 4.0), share = 1;
  for (int i = 0; i < 6; i++) {
    fac *= 4.0;
    std::vector<double> sig(D);
    for (int d = 0; d < D; d++) sig[d] = scales[d] / 100.0 / fac * 400.0;
    gset.push_back(new gaussian_prop(sig, 0.2));
    share *= 2;
    gshares.push_back(share);
  }
  proposal_distribution_set prop(gset, gshares);
  ptmcmc_sampler mcmc;
  mcmc.set("nsteps", "300"); mcmc.set("pt", "6"); mcmc.set("pt_Tmax", "50"); mcmc.set("save_every", "2");
  mcmc.set("nevery", "100"); mcmc.set("nskip", "4"); mcmc.set("pt_dump_n", "2"); mcmc.set("pt_swap_rate", "0.3");
  if (!mcmc.parse(argc - 2, argv + 2)) { printf("bad option\n"); return 2; }
  mcmc.setup(like);
  mcmc.select_proposal(prop);
  if (wrap) mcmc.set_prop_test_sizes(2048, 10, 4);
  else mcmc.set_prop_test_sizes(512, 5, 2);
  mcmc.initialize();
  mcmc.run(argv[2]);
  return 0;
}

int main(int argc, char** argv) {
  const std::string which = argc > 1 ? argv[1] : "native", path = argc > 2 ? argv[2] : "";
  if (which == "sampler" || which == "sampler_wrap") return sampler_run(argc, argv, which == "sampler_wrap");
  stateSpace space(D);
  space.set_names(std::vector<std::string>{"a", "b", "c"});
  space.set_bound(0, boundary(boundary::wrap, boundary::wrap, 0.0, 2 * M_PI));
  space.set_bound(1, boundary(boundary::limit, boundary::open, -0.6, INFINITY));
  std::valarray<double> centre(CENTRE, D);
  if (which == "seam") centre[0] = 0.5;   // 1.25 sigma from the seam at 0
  gaussian_dist_product target(&space, centre, std::valarray<double>(SIGMA, D));
  gaussian_prop native(std::vector<double>{0.7 * SIGMA[0], 0.7 * SIGMA[1], 0.7 * SIGMA[2]});
  kernel_proposal symmetric(false), contraction(true);
  host_symmetric host;
  proposal_distribution* p = which == "device" ? (proposal_distribution*)&symmetric : which == "contraction" ? (proposal_distribution*)&contraction
                           : which == "host_err" || which == "host" ? (proposal_distribution*)&host : (proposal_distribution*)&native;
  proposal_tester tester(*p, target, false, path, std::vector<int>(), 20191);
  const double err = which == "native_err" || which == "host_err" ? 0.5 : 0.0;
  const bool ok = tester.test(which == "host_err" || which == "host" ? 256 : NSAMP, NCYC, NTRY, err, 0.005);
  if (!ok) { printf("RESULT refused\n"); return 0; }
  printf("RESULT accept=%.6f moved=%d alt_fkl=%.17g fkl_redraw_max=%.17g kl=%s fkl=%s\n", tester.last_accept, tester.last_target != tester.last_transformed ? 1 : 0,
         tester.last_alt_fkl, tester.last_fkl_redraw_max, tester.last_kl->pass ? "PASS" : "FAIL", tester.last_fkl->pass ? "PASS" : "FAIL");
  return 0;
}
