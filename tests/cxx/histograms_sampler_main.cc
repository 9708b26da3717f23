// The sampler's corner file (ptmcmc_gpu.hh: ptmcmc_sampler --corner_out / --corner_bins / --corner_range) on a 3-dimensional Gaussian
// target with the default proposal recipe.  Checked by tests/test_gpu_histograms_facade.py.
//   usage: histograms_sampler <outbase> [--option=value ...]
//   stdout: the sampler's own; then, where the run's histograms were counted on the device, the same rung, window, ranges and bins
//           asked of the engine directly (ptm_quantiles, ptm_histograms): "engine <N> <nrows> <nbins>", "engine_lo ...",
//           "engine_hi ..." (%.17g), per parameter "engine_h1 ...", and the cold chains' saved rows of the window, read back from the
//           ring (the newest row last): per replica and row "cold <replica> ..." (%.17g)
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
  if (cc->histograms_ran_on_device()) {
    const int nrows = (int)((1.0 - mcmc.num("burn_frac")) * cc->rhat_rows_available(0));
    std::string bins_text, range_text;
    *mcmc.optValue("corner_bins") >> bins_text;
    *mcmc.optValue("corner_range") >> range_text;
    const int nbins = ptmcmc_sampler::parse_corner_bins(bins_text);
    const std::vector<double> probs = ptmcmc_sampler::corner_probs(ptmcmc_sampler::parse_corner_range(range_text));
    std::vector<double> q(2 * D);
    int64_t n = 0;
    if (ptm_quantiles(cc->engine(), 0, D, nrows, 2, probs.data(), q.data(), nullptr, nullptr, &n)) { printf("%s\n", ptm_last_error()); return 1; }
    std::vector<double> lo(q.begin(), q.begin() + D), hi(q.begin() + D, q.end());
    for (int i = 0; i < D; i++) ptmcmc_sampler::widen_equal_range(lo[(size_t)i], hi[(size_t)i]);
    std::vector<int64_t> h1((size_t)D * nbins);
    if (ptm_histograms(cc->engine(), 0, D, nrows, nbins, lo.data(), hi.data(), h1.data(), nullptr, nullptr, nullptr, &n)) { printf("%s\n", ptm_last_error()); return 1; }
    printf("engine %lld %d %d\n", (long long)n, nrows, nbins);
    printf("engine_lo");
    for (int i = 0; i < D; i++) printf(" %.17g", lo[(size_t)i]);
    printf("\nengine_hi");
    for (int i = 0; i < D; i++) printf(" %.17g", hi[(size_t)i]);
    printf("\n");
    for (int i = 0; i < D; i++) {
      printf("engine_h1");
      for (int k = 0; k < nbins; k++) printf(" %lld", (long long)h1[(size_t)i * nbins + k]);
      printf("\n");
    }
    // the read-back cold chains over the same window (ptm_get_history_chains: what a user of the commit before had to bin)
    const int W = cc->replicas();
    const size_t HC = (size_t)cc->history_rungs() * W, cap = (size_t)cc->history_rows();
    std::vector<double> X(cap * HC * D);
    std::vector<int32_t> meta(cap * HC * 4);
    std::vector<int64_t> nh((size_t)mcmc.num("pt") * W);
    if (ptm_get_history_chains(cc->engine(), 0, W, X.data(), nullptr, nullptr, meta.data(), nullptr) || ptm_get_array(cc->engine(), PTM_ARR_NHIST, nh.data())) { printf("%s\n", ptm_last_error()); return 1; }
    const int save_every = (int)mcmc.num("save_every");
    for (int w = 0; w < W; w++) {
      const long long newest = rhat_estimator::newest_row(nh[(size_t)w], save_every);
      for (int i = 0; i < nrows; i++) {
        const long long row = newest - nrows + 1 + i;
        const size_t o = (size_t)(row % (long long)cap) * HC + (size_t)w;
        if (row < 1 || meta[4 * o + 3] != (int32_t)row) { printf("cold row missing\n"); return 1; }
        printf("cold %d", w);
        for (int f = 0; f < D; f++) printf(" %.17g", X[o * D + f]);
        printf("\n");
      }
    }
  }
  return 0;
}
