// rhat_probe.cc -- times split R-hat of the cold rung at a population shape: ptm_rhat on the device's own ring against the path a
// caller had before it, the read-back of that rung's ring (ptm_get_history_chains) plus the host estimator (rhat_estimator).
// Prints one JSON object; profiles/rhat_device.json holds it beside the per-kernel times of a run under a kernel trace.
//   build: g++ -std=c++11 -O2 -ffp-contract=off -Iinclude -Iptmcmc_amd/host tools/rhat_probe.cc -Lptmcmc_amd -lptm_engine -Wl,-rpath,$PWD/ptmcmc_amd -pthread
//   usage: rhat_probe [replicas] [steps] [dim] [host: 0|1] [repeats]      (default 16384 1000 32 1 5)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ptmcmc_gpu.hh"
using namespace ptmgpu;

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char** argv) {
  const int W = argc > 1 ? atoi(argv[1]) : 16384, nsteps = argc > 2 ? atoi(argv[2]) : 1000, D = argc > 3 ? atoi(argv[3]) : 32;
  const bool host = argc > 4 ? atoi(argv[4]) != 0 : true;
  const int repeats = argc > 5 ? atoi(argv[5]) : 5, Nt = 2;
  stateSpace space(D);
  std::vector<std::string> names;
  for (int i = 0; i < D; i++) names.push_back("p" + std::to_string(i));
  space.set_names(names);
  std::vector<double> P((size_t)D * D, 0.0);
  for (int i = 0; i < D; i++) { P[(size_t)i * D + i] = 1.0 + 0.1 * i; if (i + 1 < D) P[(size_t)i * D + i + 1] = P[(size_t)(i + 1) * D + i] = 0.3; }
  gaussian_likelihood like(P, 0.0);
  like.basic_setup(&space, std::vector<std::string>((size_t)D, "uni"), std::vector<double>((size_t)D, 0.0), std::vector<double>((size_t)D, 20.0));
  gaussian_prop prop(std::vector<double>((size_t)D, 0.3), 0.0);
  parallel_tempering_chains ptc(Nt, 10.0, 0.1, 1);
  ptc.set_replicas(W);
  const int cap = nsteps + 2;
  ptc.keep_history(cap, 1);
  ptc.initialize(&like, like.getObjectPrior().get(), 1);
  ptc.set_proposal(prop);
  ptc.step_n(nsteps);
  ptm_engine* eng = ptc.engine();
  int nrows = ptc.rhat_rows_available(0);
  nrows -= nrows % 2;

  const size_t nf = (size_t)D, ns = 2 * (size_t)W * nf;
  std::vector<double> rhat(nf), mean(nf), within(nf), between(nf), sm(ns), sv(ns);
  double dev_ms = 1e300, dev_events_ms = 1e300;
  for (int k = 0; k < repeats; k++) {
    float ev = 0;
    ptm_check(ptm_timer_start(eng), "timer");
    const double t0 = now_ms();
    ptm_check(ptm_rhat(eng, 0, D, nrows, rhat.data(), mean.data(), within.data(), between.data(), nullptr, nullptr), "ptm_rhat");
    const double t1 = now_ms();
    ptm_check(ptm_timer_stop(eng, &ev), "timer");
    if (t1 - t0 < dev_ms) dev_ms = t1 - t0;
    if (ev < dev_events_ms) dev_events_ms = ev;
  }
  double mx = 0;
  for (size_t f = 0; f < nf; f++) if (!(rhat[f] <= mx)) mx = rhat[f];
  printf("{\"shape\": {\"dim\": %d, \"n_rungs\": %d, \"replicas\": %d, \"steps\": %d, \"add_every_n\": 1, \"ring_rows\": %d, \"rung\": 0, \"nfeat\": %d, \"nrows\": %d},\n", D, Nt, W, nsteps, cap, D, nrows);
  printf(" \"ptm_rhat_ms_host_clock_best_of_%d\": %.4f, \"ptm_rhat_ms_stream_events_best\": %.4f, \"rhat_max\": %.17g,\n", repeats, dev_ms, dev_events_ms, mx);
  printf(" \"sequence_kernel_algorithmic_bytes\": %.0f", 2.0 * nrows * W * nf * 8.0);
  if (host) {
    const size_t HC = (size_t)W, n = (size_t)cap * HC;
    double t0 = now_ms();
    std::vector<double> X(n * D);
    std::vector<int32_t> meta(n * 4, -1);
    const double t_alloc = now_ms() - t0;
    t0 = now_ms();
    ptm_check(ptm_get_history_chains(eng, 0, W, X.data(), nullptr, nullptr, meta.data(), nullptr), "read-back");
    const double t_read = now_ms() - t0;
    std::vector<int64_t> nh((size_t)Nt * W);
    ptm_check(ptm_get_array(eng, PTM_ARR_NHIST, nh.data()), "nhist");
    std::vector<long long> newest((size_t)W);
    for (int w = 0; w < W; w++) newest[(size_t)w] = rhat_estimator::newest_row(nh[(size_t)w], 1);
    t0 = now_ms();
    const rhat_estimator::result r = rhat_estimator::estimate(W, D, nrows, newest.data(), [&](int w, long long row, std::vector<double>& v) {
      const size_t o = (size_t)(row % (long long)cap) * HC + w;
      if (meta[4 * o + 3] != (int32_t)row) return false;
      v.assign(X.begin() + o * D, X.begin() + (o + 1) * D);
      return true;
    });
    const double t_twin = now_ms() - t0;
    bool same = r.complete;
    for (size_t f = 0; f < nf; f++) same = same && r.rhat[f] == rhat[f] && r.within[f] == within[f] && r.between[f] == between[f];
    printf(",\n \"host_path\": {\"alloc_ms\": %.1f, \"ptm_get_history_chains_ms\": %.1f, \"rhat_estimator_one_core_ms\": %.1f, \"read_back_bytes\": %.0f, \"same_bits_as_device\": %s}",
           t_alloc, t_read, t_twin, (double)n * (D * 8.0 + 16.0), same ? "true" : "false");
  }
  printf("}\n");
  return 0;
}
