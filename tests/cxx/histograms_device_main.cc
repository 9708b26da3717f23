// The facade's corner-plot histograms on the device (ptmcmc_gpu.hh: parallel_tempering_chains::posterior_histograms) against its own
// host estimator: a small ladder of 70 replicas with a saved history.  Checked by tests/test_gpu_histograms_facade.py.
//   usage: histograms_device [nsteps] [many|hostprop]
//   stdout: "counts <add_state calls of each replica's chain on rung 1>", then per query q (rung, nfeat, nrows, nbins, pairs)
//           "query <q> <rung> <nfeat> <nrows> <nbins> <pairs> count=<N> device=<0|1>" (PTM_HOST_HISTOGRAMS=1 keeps the host path),
//           "lo <q> ...", "hi <q> ..." (%.17g), "below <q> ...", "above <q> ...", per feature "h1 <q> ...", per pair "h2 <q> ..."
//           The ranges are quantiles of the sample itself: the minimum and maximum, or the 5% and 95% points.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ptmcmc_gpu.hh"
using namespace ptmgpu;

static void line(const char* tag, int q, const double* v, size_t n) {
  printf("%s %d", tag, q);
  for (size_t i = 0; i < n; i++) printf(" %.17g", v[i]);
  printf("\n");
}
static void line(const char* tag, int q, const int64_t* v, size_t n) {
  printf("%s %d", tag, q);
  for (size_t i = 0; i < n; i++) printf(" %lld", (long long)v[i]);
  printf("\n");
}

int main(int argc, char** argv) {
  const int nsteps = argc > 1 ? atoi(argv[1]) : 2000;
  // "many": an 8-rung ladder with five exchange candidates per step (the replicas' windows on rung 1 differ); "hostprop": host-side
  // proposals, the history is the host mirror, with the initial rows in front of the start state's; else one candidate per step
  const std::string mode = argc > 2 ? argv[2] : "";
  const bool many = mode == "many", hostprop = mode == "hostprop";
  const int D = 3, Nt = many ? 8 : 3, W = 70, add_every = 2;
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
  const struct { int rung, nfeat, nrows, nbins; bool pairs, whole; } queries[] = {{0, 3, 500, 20, true, true}, {1, 2, 250, 7, true, false}, {0, 3, -1, 128, true, false}, {1, 1, 1, 1, true, true},
                                                                                 {0, 3, 300, 20, false, false}};
  for (int q = 0; q < 5; q++) {
    const int nf = queries[q].nfeat;
    const std::vector<double> probs = queries[q].whole ? std::vector<double>{0.0, 1.0} : std::vector<double>{0.05, 0.95};
    const quantile_estimator::result ends = ptc.posterior_quantiles(probs, queries[q].rung, nf, queries[q].nrows);
    std::vector<double> lo(ends.q.begin(), ends.q.begin() + nf), hi(ends.q.begin() + nf, ends.q.begin() + 2 * nf);
    for (int f = 0; f < nf; f++)
      if (lo[(size_t)f] == hi[(size_t)f]) { lo[(size_t)f] -= 0.5; hi[(size_t)f] += 0.5; }
    const histogram_estimator::result r = ptc.posterior_histograms(lo, hi, queries[q].nbins, queries[q].rung, nf, queries[q].nrows, queries[q].pairs);
    printf("query %d %d %d %d %d %d count=%lld device=%d\n", q, queries[q].rung, nf, queries[q].nrows, queries[q].nbins, queries[q].pairs ? 1 : 0, r.count, ptc.histograms_ran_on_device() ? 1 : 0);
    const size_t F = (size_t)nf, B = (size_t)queries[q].nbins;
    line("lo", q, r.lo.data(), F);
    line("hi", q, r.hi.data(), F);
    line("below", q, r.below.data(), F);
    line("above", q, r.above.data(), F);
    for (size_t f = 0; f < F; f++) line("h1", q, r.h1.data() + f * B, B);
    for (size_t p = 0; p * B * B < r.h2.size(); p++) line("h2", q, r.h2.data() + p * B * B, B * B);
  }
  return 0;
}
