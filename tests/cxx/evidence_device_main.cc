// The facade's log-evidence (ptmcmc_gpu.hh: parallel_tempering_chains with do_evid) on a small ladder: a statistics bin of 500 steps,
// stepped in calls of 300 so that the engine calls are cut at the bin boundaries.  Checked by tests/test_gpu_evidence_facade.py.
//   usage: evidence_device <nsteps> <replicas> [noevid]      (PTM_HOST_EVIDENCE=1 keeps the host path)
//   stdout: the ladder's own lines (replica 0's, the reference's), after every call that closed a bin
//           "bin <epochs> <replica> ev <%.17g> best <%.17g> records <level sizes and their last entries %.17g>", at the end
//           "state <chain> <llike %.17g> <parameters %.17g>" of every chain and the status text.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "ptmcmc_gpu.hh"
using namespace ptmgpu;

int main(int argc, char** argv) {
  const int nsteps = argc > 1 ? atoi(argv[1]) : 3500, W = argc > 2 ? atoi(argv[2]) : 1;
  const bool evid = !(argc > 3 && std::string(argv[3]) == "noevid");
  const int D = 3, Nt = 4;
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
  parallel_tempering_chains ptc(Nt, 30.0, 0.3, 1, evid, true);
  ptc.set_replicas(W);
  ptc.set_stats_bin(500);
  ptc.initialize(&like, like.getObjectPrior().get(), 1);
  ptc.set_proposal(prop);
  int seen = 0;
  for (int done = 0; done < nsteps;) {
    const int k = std::min(300, nsteps - done);
    ptc.step_n(k);
    done += k;
    if (ptc.evidence_epochs() == seen) continue;
    seen = ptc.evidence_epochs();
    std::cout << std::flush;
    for (int w = 0; w < W; w++) {
      printf("bin %d %d ev %.17g best %.17g records", seen, w, ptc.lastEvidence(w), ptc.bestEvidenceErr(w));
      for (const std::vector<double>& level : ptc.evidenceRecords(w).levels()) printf(" %d:%.17g", (int)level.size(), level.empty() ? 0.0 : level.back());
      printf("\n");
    }
    fflush(stdout);
  }
  std::vector<double> X((size_t)Nt * W * D), ll((size_t)Nt * W);
  if (ptm_get_states(ptc.engine(), X.data()) || ptm_get_array(ptc.engine(), PTM_ARR_LLIKE, ll.data())) { printf("%s\n", ptm_last_error()); return 1; }
  for (size_t c = 0; c < ll.size(); c++) printf("state %d %.17g %.17g %.17g %.17g\n", (int)c, ll[c], X[c * D], X[c * D + 1], X[c * D + 2]);
  fflush(stdout);
  std::cout << ptc.status() << std::flush;
  return 0;
}
