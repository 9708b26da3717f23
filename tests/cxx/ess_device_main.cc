// The facade's effective-sample-size report on the device (ptmcmc_gpu.hh: report_effective_samples, report_effective_samples_all)
// against its own host estimator: a small ladder of 5 replicas with a saved history.  Checked by tests/test_gpu_ess_facade.py.
//   usage: ess_device [nsteps] [many]
//   stdout: "counts <add_state calls of each replica's cold chain>", then "cold <query> <ess> <length> device=<0|1>" per query (PTM_HOST_ESS=1 keeps the host path), then per replica
//           "replica <query> <w> <ess> <length> host <ess> <length>": the population entry point beside ess_estimator run here on that
//           replica's rows as ptm_get_history_chains returns them
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ptmcmc_gpu.hh"
using namespace ptmgpu;

int main(int argc, char** argv) {
  const int nsteps = argc > 1 ? atoi(argv[1]) : 4000;
  // "many": an 8-rung ladder with five exchange candidates per step (rungs above the coldest are then exchanged twice in some steps
  // and make extra add_state calls; the coldest never is); else one candidate per step
  const bool many = argc > 2 && std::string(argv[2]) == "many";
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
  ptc.keep_history(nsteps / add_every + 2000, 1);
  ptc.initialize(&like, like.getObjectPrior().get(), 1);
  ptc.set_proposal(prop);
  ptc.step_n(nsteps);

  std::vector<int64_t> nh((size_t)Nt * W);
  if (ptm_get_array(ptc.engine(), PTM_ARR_NHIST, nh.data())) { printf("%s\n", ptm_last_error()); return 1; }
  printf("counts");
  for (int w = 0; w < W; w++) printf(" %lld", (long long)nh[(size_t)w]);
  printf("\n");
  const struct { int width, every; double limit; } queries[] = {{100, 2, -1.0}, {200, -1, -1.0}, {100, 1, 0.4}};
  for (int q = 0; q < 3; q++) {
    const std::pair<double, int> cold = ptc.report_effective_samples(-1, queries[q].width, queries[q].every, queries[q].limit, false);
    printf("cold %d %.17g %d device=%d\n", q, cold.first, cold.second, ptc.ess_ran_on_device() ? 1 : 0);
    const std::vector<std::pair<double, int> > all = ptc.report_effective_samples_all(-1, queries[q].width, queries[q].every, queries[q].limit);
    for (int w = 0; w < W; w++) {
      const size_t cap = (size_t)nsteps / add_every + 2000, HC = W;
      std::vector<double> X(cap * HC * D);
      std::vector<int32_t> meta(cap * HC * 4, -1);
      if (ptm_get_history_chains(ptc.engine(), w, 1, X.data(), nullptr, nullptr, meta.data(), nullptr)) { printf("%s\n", ptm_last_error()); return 1; }
      ess_estimator est((int)nh[(size_t)w], D, [&](int step, std::vector<double>& row) {
        const int idx = 1 + step / add_every;
        const size_t o = (size_t)(idx % (int)cap) * HC + w;
        if (meta[4 * o + 3] != idx) return false;
        row.assign(X.begin() + o * D, X.begin() + (o + 1) * D);
        return true;
      });
      const std::pair<double, int> host = est.report(queries[q].width, queries[q].every, queries[q].limit, ptc.subchain(0, w)->size(), 1);
      printf("replica %d %d %.17g %d host %.17g %d\n", q, w, all[(size_t)w].first, all[(size_t)w].second, host.first, host.second);
    }
  }
  return 0;
}
