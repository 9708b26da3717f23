// The sampler's covariance file (ptmcmc_gpu.hh: ptmcmc_sampler --covariance_out / --covariance_file) on a 3-dimensional Gaussian
// target with the default proposal recipe.  Checked by tests/test_gpu_moments_facade.py.
//   usage: moments_sampler <outbase> [--option=value ...]
//   stdout: the sampler's own; then, where the run's moments were estimated on the device, the same rung and window asked of the
//           engine directly (ptm_moments): "engine <N> <nrows>", "engine_mean ...", per row "engine_cov ..." (%.17g)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ptmcmc_gpu.hh"
using namespace ptmgpu;

int main(int argc, char** argv) {
  if (argc < 2) { printf("usage: %s <outbase> [--option=value ...]\n", argv[0]); return 2; }
  const int D = 3;
  std::vector<double> P = {2.0, 0.6, 0.0, 0.6, 1.0, -0.3, 0.0, -0.3, 1.5};   // precision of the target
  stateSpace space(D);
  space.set_names(std::vector<std::string>{"a", "b", "c"});
  gaussian_likelihood like(P, 0.0);
  std::vector<std::string> types(D, "uni");
  std::vector<double> centers(D, 0.0), scales(D, 20.0);
  like.basic_setup(&space, types, centers, scales);
  ptmcmc_sampler mcmc;
  mcmc.set("nsteps", "2000"); mcmc.set("pt", "6"); mcmc.set("pt_Tmax", "50"); mcmc.set("save_every", "2");
  mcmc.set("nevery", "500"); mcmc.set("nskip", "4"); mcmc.set("pt_dump_n", "2"); mcmc.set("pt_swap_rate", "0.3");
  if (!mcmc.parse(argc - 1, argv + 1)) { printf("bad option\n"); return 2; }
  mcmc.setup(like);
  mcmc.select_proposal();
  mcmc.initialize();
  mcmc.run(argv[1]);
  parallel_tempering_chains* cc = mcmc.chains();
  if (cc->moments_ran_on_device()) {
    const int nrows = (int)((1.0 - mcmc.num("burn_frac")) * cc->rhat_rows_available(0));
    std::vector<double> mean(D), cov(D * D);
    int64_t n = 0;
    if (ptm_moments(cc->engine(), 0, D, nrows, mean.data(), cov.data(), nullptr, nullptr, &n)) { printf("%s\n", ptm_last_error()); return 1; }
    printf("engine %lld %d\nengine_mean", (long long)n, nrows);
    for (int i = 0; i < D; i++) printf(" %.17g", mean[i]);
    printf("\n");
    for (int i = 0; i < D; i++) {
      printf("engine_cov");
      for (int j = 0; j < D; j++) printf(" %.17g", cov[i * D + j]);
      printf("\n");
    }
  }
  return 0;
}
