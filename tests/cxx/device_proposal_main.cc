// A device_proposal through the facade (ptmcmc_gpu.hh), beside a device_likelihood: the whole step stays on the device.  The
// proposal wraps the launchers of examples/scripted_device_proposal.hip; its host draw() is the same arithmetic in C++ (every
// operation one exactly rounded +, * or conversion: build with -ffp-contract=off), so PTM_DEVICE_PROPOSAL=1 and =0 write the same chain
// files.  The likelihood is a diagonal quadratic, on the device a kernel with the host function's operations in the host's order.
// Compiled as HIP (-x hip).  Checked by tests/test_gpu_device_proposals.py.
//   usage: device_proposal <outbase> [--option=value ...]
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ptmcmc_gpu.hh"
using namespace ptmgpu;

// examples/scripted_device_proposal.hip
struct scripted_proposal_user {
  const double* scale_dev;
  int32_t* accepted_out_dev;
  int32_t* rung_out_dev;
  int32_t* walker_out_dev;
  int32_t* count_out_dev;
  uint64_t calls, result_calls;
  uint64_t last_step[4];
};
extern "C" void scripted_propose_device(void* user, void* stream, int n_rows, int dim, const double* X_cur_dev, const int32_t* rung_dev,
                                        const int32_t* walker_dev, const int32_t* count_dev, uint64_t step, double* X_prop_dev,
                                        double* log_hastings_dev, int32_t* type_dev, int32_t* valid_dev);

static const int D = 5, NT = 6;

// ---- the likelihood: -1/2 sum_d ((0.7 + 0.1 d) x_d)^2, summed in index order
__host__ __device__ inline double quad_like(const double* x, int dim) {
  double acc = 0.0;
  for (int d = 0; d < dim; d++) {
    const double t = x[d] * (0.7 + 0.1 * d);
    acc = acc + t * t;
  }
  return -0.5 * acc;
}
__global__ __launch_bounds__(256) void quad_like_kernel(int n, int dim, const double* __restrict__ X, double* __restrict__ out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < n) out[k] = quad_like(X + (size_t)k * dim, dim);
}
static double quad_like_host(void*, const state& s) {
  const std::vector<double> x = s.get_params_vector();
  return quad_like(x.data(), (int)x.size());
}
class quad_device_like : public device_likelihood {
 public:
  void evaluate_log_device(void* stream, int n_rows, int dim, const double* X_dev, const int32_t*, double* out_dev) override {
    if (n_rows > 0) hipLaunchKernelGGL(quad_like_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_rows, dim, X_dev, out_dev);
  }
};

// ---- the proposal: scripted_proposal of tests/test_gpu_host_proposals.py
static uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static double uniform_of(uint64_t base, int col) {
  const uint64_t z = mix64(base + (uint64_t)(col + 1) * 0xD6E8FEB86659FD93ull);
  return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

class scripted_device_proposal : public device_proposal {
  std::vector<double> scale;
  double* scale_dev = nullptr;
  scripted_proposal_user user;

 public:
  explicit scripted_device_proposal(const std::vector<double>& scale_of_rung) : scale(scale_of_rung) {
    if (hipMalloc((void**)&scale_dev, scale.size() * sizeof(double)) != hipSuccess ||
        hipMemcpy(scale_dev, scale.data(), scale.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
      std::cout << "scripted_device_proposal: no device buffer" << std::endl;
      exit(1);
    }
    user = scripted_proposal_user();
    user.scale_dev = scale_dev;
  }
  ~scripted_device_proposal() override { (void)hipFree(scale_dev); }
  proposal_distribution* clone() const override { return new scripted_device_proposal(scale); }
  std::string show() override { return "ScriptedDeviceProposal()"; }
  void draw_device(void* stream, int n_rows, int dim, const double* X_cur_dev, const int32_t* rung_dev, const int32_t* walker_dev,
                   const int32_t* count_dev, uint64_t step, double* X_prop_dev, double* log_hastings_dev, int32_t* type_dev,
                   int32_t* valid_dev) override {
    scripted_propose_device(&user, stream, n_rows, dim, X_cur_dev, rung_dev, walker_dev, count_dev, step, X_prop_dev, log_hastings_dev, type_dev, valid_dev);
  }
  // the host path: one chain, the same numbers (the caller is the chain's view: its id is replica * rungs + rung)
  state draw(state& s, chain* caller) override {
    const int dim = s.size(), id = caller->get_id();
    const int rung = id % NT, walker = id / NT;
    const uint64_t step = (uint64_t)caller->getStep();
    const uint64_t base = (uint64_t)rung * 0x9E3779B97F4A7C15ull + (uint64_t)walker * 0xC2B2AE3D27D4EB4Full + step * 0x165667B19E3779F9ull;
    std::vector<double> x(dim);
    const bool big = uniform_of(base, dim) < 0.04;
    for (int d = 0; d < dim; d++) {
      const double u = uniform_of(base, d);
      double p = s.get_param(d) + scale[rung] * (2 * u - 1);
      if (big) p = p * 40.0 + 7.0;
      x[d] = p;
    }
    const double u1 = uniform_of(base, dim + 1), u2 = uniform_of(base, dim + 2), u3 = uniform_of(base, dim + 3);
    double h = 1.6 * (u1 - 0.5);
    if (u2 < 0.05) h = 0.0;
    if (u2 > 0.97) h = NAN;
    log_hastings = h;
    last_type = (int)(u3 * 5);
    if (u3 > 0.03) return s.moved_to(x);
    return state::from_engine(nullptr, x.data(), dim);   // (no space: an invalid state)
  }
  unsigned long long device_calls() const { return user.calls; }
};

int main(int argc, char** argv) {
  if (argc < 2) { printf("usage: %s <outbase> [--option=value ...]\n", argv[0]); return 2; }
  stateSpace space(D);
  std::vector<std::string> names, types(D, "uni");
  for (int i = 0; i < D; i++) names.push_back("p" + std::to_string(i));
  space.set_names(names);
  std::vector<double> centers(D, 0.0), scales(D, 20.0);
  quad_device_like like;
  like.register_evaluate_log(quad_like_host);
  like.basic_setup(&space, types, centers, scales);
  std::vector<double> scale(NT);
  for (int i = 0; i < NT; i++) scale[i] = 0.8 * std::pow(1.5, i);
  scripted_device_proposal prop(scale);
  ptmcmc_sampler mcmc;
  mcmc.set("nsteps", "400"); mcmc.set("pt", std::to_string(NT)); mcmc.set("pt_Tmax", "50"); mcmc.set("save_every", "2");
  mcmc.set("nevery", "200"); mcmc.set("nskip", "2"); mcmc.set("pt_dump_n", "3"); mcmc.set("pt_swap_rate", "0.3");
  if (!mcmc.parse(argc - 1, argv + 1)) { printf("bad option\n"); return 2; }
  mcmc.setup(like);
  mcmc.select_proposal(prop);
  mcmc.initialize();
  mcmc.run(argv[1]);
  printf("%s", mcmc.chains()->status().c_str());
  printf("step kernel: %s\n", ptm_step_kernel_name(mcmc.chains()->engine()));
  printf("device_proposal path: %s\n", mcmc.chains()->draws_user_proposal_on_device() ? "device" : "host");
  return 0;
}
