// The facade's proposal adaptation (ptmcmc_gpu.hh: parallel_tempering_chains::adapt_gaussian_proposals) on the device against its own
// host route (PTM_HOST_PROPOSAL_ADAPT=1): a ladder of 4 rungs x 70 replicas with every rung recorded, adapted twice during the run.
// Checked by tests/test_gpu_prop_adapt_facade.py.
//   usage: prop_adapt_device <outbase> dense|diag|hostprop
//   writes <outbase>_c<w>_t<rung>.dat (dumpChain) for rungs 0 and 3 of replicas 0 and 69
//   stdout: per adaptation "adapt rows=<rows> rungs=<n> set=<k> not_finite=<a> not_positive=<b> device=<0|1>"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "ptmcmc_gpu.hh"
using namespace ptmgpu;

int main(int argc, char** argv) {
  if (argc < 3) { printf("usage: %s <outbase> dense|diag|hostprop\n", argv[0]); return 2; }
  const std::string base = argv[1], mode = argv[2];
  const int D = 3, Nt = 4, W = 70;
  stateSpace space(D);
  space.set_names(std::vector<std::string>{"a", "b", "c"});
  std::vector<double> P = {2.0, 0.6, 0.0, 0.6, 1.0, -0.3, 0.0, -0.3, 1.5};
  gaussian_likelihood like(P, 0.0);
  like.basic_setup(&space, new uniform_dist_product(&space, std::valarray<double>{-20, -20, -20}, std::valarray<double>{20, 20, 20}));
  std::vector<double> sig(D, 1.0), cov = {1.0, 0.2, 0.0, 0.2, 1.0, 0.1, 0.0, 0.1, 1.0};
  gaussian_prop diag(sig, 0.0), dense(cov, D, 0.0);
  parallel_tempering_chains ptc(Nt, 30.0, 0.3, 1);
  ptc.set_replicas(W);
  if (mode == "hostprop") {
    differential_evolution* de = new differential_evolution(0.3, 0.3, 1e-4, 0.0, 0.0);
    de->reduce_gamma(1.0);
    proposal_distribution_set* set = new proposal_distribution_set(std::vector<proposal_distribution*>{de, new gaussian_prop(sig, 0.0)}, std::vector<double>{0.5, 0.5});
    ptc.use_host_proposals(true);
    ptc.initialize(&like, like.getObjectPrior().get(), 20 * D);
    ptc.set_proposal(*set);
  } else {
    ptc.keep_history(1000, 0);
    ptc.initialize(&like, like.getObjectPrior().get(), 1);
    ptc.set_proposal(mode == "diag" ? (proposal_distribution&)diag : (proposal_distribution&)dense);
  }
  const int legs[3] = {200, 200, 300};
  for (int k = 0; k < 3; k++) {
    ptc.step_n(mode == "hostprop" ? 20 : legs[k]);
    if (k == 2) break;
    const parallel_tempering_chains::proposal_adapt_result r = k == 0 ? ptc.adapt_gaussian_proposals(150, 0.9) : ptc.adapt_gaussian_proposals();
    printf("adapt rows=%d rungs=%d set=%d not_finite=%d not_positive=%d device=%d\n", r.rows, r.rungs, r.set, r.not_finite, r.not_positive,
           ptc.proposal_adapt_ran_on_device() ? 1 : 0);
  }
  if (mode == "hostprop") return 0;
  const int rungs[2] = {0, 3}, reps[2] = {0, 69};
  for (int a = 0; a < 2; a++)
    for (int b = 0; b < 2; b++) {
      std::ostringstream name;
      name << base << "_c" << reps[a] << "_t" << rungs[b] << ".dat";
      std::ofstream out(name.str().c_str());
      out.precision(17);
      ptc.dumpChain(rungs[b], out, 0, 1, reps[a]);
    }
  return 0;
}
