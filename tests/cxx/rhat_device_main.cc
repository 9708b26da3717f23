// The facade's split R-hat on the device (ptmcmc_gpu.hh: parallel_tempering_chains::split_rhat) against its own host estimator: a
// small ladder of 5 replicas with a saved history.  Checked by tests/test_gpu_rhat_facade.py.
//   usage: rhat_device [nsteps] [many|hostprop]
//   stdout: "counts <add_state calls of each replica's chain on rung 1>", then per query q (rung, nfeat, nrows)
//           "query <q> <rung> <nfeat> <nrows> device=<0|1>" (PTM_HOST_RHAT=1 keeps the host path), per feature
//           "feature <q> <f> <rhat> <mean> <within> <between>" and per sequence and feature "sequence <q> <k> <f> <mean> <var>" (%.17g)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ptmcmc_gpu.hh"
using namespace ptmgpu;

int main(int argc, char** argv) {
  const int nsteps = argc > 1 ? atoi(argv[1]) : 4000;
  // "many": an 8-rung ladder with five exchange candidates per step (rungs above the coldest are then exchanged twice in some steps
  // and make extra add_state calls: the replicas' windows on rung 1 differ); "hostprop": host-side proposals, the history is the
  // host mirror, with the initial rows in front of the start state's; else one candidate per step
  const std::string mode = argc > 2 ? argv[2] : "";
  const bool many = mode == "many", hostprop = mode == "hostprop";
  const int D = 3, Nt = many ? 8 : 3, W = 5, add_every = 2;
  stateSpace space(D);
  space.set_names(std::vector<std::string>{"a", "b", "c"});
  std::vector<double> P(D * D, 0.0);
  const double prec[3] = {1.0, 0.5, 2.0};
  for (int i = 0; i < D; i++) P[i * D + i] = prec[i];
  P[1] = P[3] = 0.3;
  gaussian_likelihood like(P, 0.0);
  like.basic_setup(&space, new uniform_dist_product(&space, std::valarray<double>{-20, -20, -20}, std::valarray<double>{20, 20, 20}));
  std::vector<double> sig(D, 1.0);
  gaussian_prop prop(sig, 0.0);
  parallel_tempering_chains ptc(Nt, 30.0, many ? 0.3 : 0.1, add_every);
  ptc.set_replicas(W);
  if (hostprop) {   // a differential evolution without a ring for it: the whole set is drawn on the host, from 20 D initial rows
    differential_evolution* de = new differential_evolution(0.3, 0.3, 1e-4, 0.0, 0.0);
    de->reduce_gamma(1.0);
    proposal_distribution_set* set = new proposal_distribution_set(std::vector<proposal_distribution*>{de, new gaussian_prop(sig, 0.0)}, std::vector<double>{0.5, 0.5});
    ptc.use_host_proposals(true);
    ptc.initialize(&like, like.getObjectPrior().get(), 20 * D);
    ptc.set_proposal(*set);
    if (!ptc.proposals_on_host()) { printf("hostprop: the proposals are not drawn on the host\n"); return 1; }
  } else {
    ptc.keep_history(nsteps / add_every + 2000, 2);
    ptc.initialize(&like, like.getObjectPrior().get(), 1);
    ptc.set_proposal(prop);
  }
  ptc.step_n(nsteps);

  std::vector<int64_t> nh((size_t)Nt * W);
  if (ptm_get_array(ptc.engine(), PTM_ARR_NHIST, nh.data())) { printf("%s\n", ptm_last_error()); return 1; }
  printf("counts");
  for (int w = 0; w < W; w++) printf(" %lld", (long long)nh[(size_t)W + w]);
  printf("\n");
  const struct { int rung, nfeat, nrows; } queries[] = {{0, 3, 1000}, {1, 2, 500}, {0, 3, -1}, {1, 1, 4}};
  for (int q = 0; q < 4; q++) {
    const int nf = queries[q].nfeat;
    const rhat_estimator::result r = ptc.split_rhat(queries[q].rung, nf, queries[q].nrows);
    printf("query %d %d %d %d device=%d\n", q, queries[q].rung, nf, queries[q].nrows, ptc.rhat_ran_on_device() ? 1 : 0);
    for (int f = 0; f < nf; f++) printf("feature %d %d %.17g %.17g %.17g %.17g\n", q, f, r.rhat[f], r.mean[f], r.within[f], r.between[f]);
    for (int k = 0; k < 2 * W; k++)
      for (int f = 0; f < nf; f++) printf("sequence %d %d %d %.17g %.17g\n", q, k, f, r.seq_mean[(size_t)k * nf + f], r.seq_var[(size_t)k * nf + f]);
  }
  return 0;
}
