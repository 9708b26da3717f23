// The sampler's proposal adaptation (ptmcmc_gpu.hh: ptmcmc_sampler --prop_cov_adapt_every / _rows / _scale) on a 3-dimensional
// Gaussian target with the default proposal recipe.  Checked by tests/test_gpu_prop_adapt_facade.py.
//   usage: prop_adapt_sampler <outbase> [--option=value ...]
//   stdout: the sampler's own (one "Proposal factors from ..." line per adaptation)
#include <cstdio>
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
  return 0;
}
