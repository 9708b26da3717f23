// The sampler's quantile file (ptmcmc_gpu.hh: ptmcmc_sampler --quantiles_out / --quantile_probs) on a 3-dimensional Gaussian target
// with the default proposal recipe.  Checked by tests/test_gpu_quantiles_facade.py.
//   usage: quantiles_sampler <outbase> [--option=value ...]
//   stdout: the sampler's own; then, where the run's quantiles were selected on the device, the same rung, window and probabilities
//           asked of the engine directly (ptm_quantiles): "engine <N> <nrows>", per probability "engine_q ..." (%.17g), and the
//           effective samples the window holds, summed over the replicas' cold chains: "ess <sum> <replicas counted>" -- a
//           replica's window of nrows * save_every steps over its own autocorrelation length (useful length / ess of
//           report_effective_samples_all)
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
  if (cc->quantiles_ran_on_device()) {
    const int nrows = (int)((1.0 - mcmc.num("burn_frac")) * cc->rhat_rows_available(0));
    const int save_every = (int)mcmc.num("save_every");
    std::string probs_text;
    *mcmc.optValue("quantile_probs") >> probs_text;
    const std::vector<double> probs = ptmcmc_sampler::parse_quantile_probs(probs_text);
    std::vector<double> q(probs.size() * D);
    int64_t n = 0;
    if (ptm_quantiles(cc->engine(), 0, D, nrows, (int)probs.size(), probs.data(), q.data(), nullptr, nullptr, &n)) { printf("%s\n", ptm_last_error()); return 1; }
    printf("engine %lld %d\n", (long long)n, nrows);
    for (size_t k = 0; k < probs.size(); k++) {
      printf("engine_q");
      for (int i = 0; i < D; i++) printf(" %.17g", q[k * D + i]);
      printf("\n");
    }
    const std::vector<std::pair<double, int> > all = cc->report_effective_samples_all(-1, save_every * 100, save_every);
    double ess = 0;
    int counted = 0;
    for (size_t w = 0; w < all.size(); w++)
      if (all[w].first > 0 && all[w].second > 0) { ess += (double)nrows * save_every / (all[w].second / all[w].first); counted++; }
    printf("ess %.17g %d\n", ess, counted);
  }
  return 0;
}
