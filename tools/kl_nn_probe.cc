// kl_nn_probe.cc -- times the exact nearest-neighbour search of the k-NN KL estimator at one shape: ptm_nn_dist2 on the device (host
// arrays in, host array out: allocation, copies, the three kernels) against the facade's kl_estimator on one core, and compares
// their bits.  Prints one JSON object per run; profiles/proposal_test.json holds them.
//   build: g++ -std=c++11 -O2 -ffp-contract=off -Iinclude -Iptmcmc_amd/host tools/kl_nn_probe.cc -Lptmcmc_amd -lptm_engine -Wl,-rpath,$PWD/ptmcmc_amd -pthread
//   usage: kl_nn_probe [n] [dim] [same_set: 0|1] [host: 0|1] [repeats]      (default 10000 6 0 1 5; both sets have n points)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ptmcmc_gpu.hh"
using namespace ptmgpu;

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char** argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 10000, dim = argc > 2 ? atoi(argv[2]) : 6;
  const bool same = argc > 3 && atoi(argv[3]) != 0, host = argc > 4 ? atoi(argv[4]) != 0 : true;
  const int repeats = argc > 5 ? atoi(argv[5]) : 5;
  // two seeded standard-normal sets (Box-Muller on a 64-bit LCG)
  unsigned long long s = 0x9E3779B97F4A7C15ull;
  auto uni = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return ((s >> 11) + 0.5) / 9007199254740992.0; };
  auto normal = [&]() { return std::sqrt(-2.0 * std::log(uni())) * std::cos(6.283185307179586 * uni()); };
  std::vector<double> P((size_t)n * dim), Q((size_t)n * dim), dev((size_t)n), cpu((size_t)n);
  for (auto& v : P) v = normal();
  for (auto& v : Q) v = 1.1 * normal();
  const double* q = same ? P.data() : Q.data();
  ptm_check(ptm_nn_dist2(-1, P.data(), n, q, n, dim, nullptr, nullptr, nullptr, same ? 1 : 0, dev.data()), "ptm_nn_dist2 (warm-up)");
  double best = 1e300, sum = 0;
  for (int k = 0; k < repeats; k++) {
    const double t0 = now_ms();
    ptm_check(ptm_nn_dist2(-1, P.data(), n, q, n, dim, nullptr, nullptr, nullptr, same ? 1 : 0, dev.data()), "ptm_nn_dist2");
    const double t = now_ms() - t0;
    if (t < best) best = t;
    sum += t;
  }
  printf("{\"n\": %d, \"dim\": %d, \"same_set\": %s, \"pair_dimensions\": %.0f, \"ptm_nn_dist2_ms_best_of_%d\": %.3f, \"ptm_nn_dist2_ms_mean\": %.3f", n, dim,
         same ? "true" : "false", (double)n * n * dim, repeats, best, sum / repeats);
  if (host) {
    const double t0 = now_ms();
    if (same) cpu = kl_estimator::all_nnd2(P.data(), n, dim);
    else
      for (int i = 0; i < n; i++) cpu[(size_t)i] = kl_estimator::one_nnd2(P.data() + (size_t)i * dim, Q.data(), n, dim);
    const double t = now_ms() - t0;
    bool same_bits = true;
    for (int i = 0; i < n; i++) same_bits = same_bits && cpu[(size_t)i] == dev[(size_t)i];
    printf(", \"kl_estimator_one_core_ms\": %.1f, \"same_bits_as_device\": %s", t, same_bits ? "true" : "false");
  }
  printf("}\n");
  return 0;
}
