// example_lisa_device.cc -- examples/example_lisa.cc with the likelihood ON THE DEVICE: the same main(), call for call, but the
// likelihood is a device_likelihood (ptmcmc_gpu.hh) whose evaluate_log_device launches the HIP kernel of
// examples/lisa_device_likelihood.hip on the engine's stream -- the step is then propose pass -> pack -> the kernel -> scatter ->
// accept pass with no host wait.  Its host evaluate_log (still required: a prior that is not a per-dimension product, host-side
// proposals, and PTM_DEVICE_LIKE=0 in the environment take the host path) launches the same kernel on one row, so both paths
// share one arithmetic and write the same chains.  best_post is the engine's best evaluated posterior (ptm_get_best_evaluated).
//   build: hipcc --offload-arch=gfx950 -std=c++17 -O2 -ffp-contract=off -Iinclude -Iptmcmc_amd/host examples/example_lisa_device.cc examples/lisa_device_likelihood.hip -Lptmcmc_amd -lptm_engine -Wl,-rpath,$PWD/ptmcmc_amd -o lisa_device
//   usage: as example_lisa; PTM_DEVICE_LIKE=0 forces the host path
#include <cmath>
#include <cstdio>
#include <ctime>
#include <vector>

#include "ptmcmc_gpu.hh"
using namespace ptmgpu;

#include <hip/hip_runtime_api.h>

// examples/lisa_device_likelihood.hip
extern "C" void lisa_loglike_device(void* user, void* stream, int n_rows, int dim, const double* X_dev, const int32_t* count_dev,
                                    double* out_llike_dev);

// the host form: the same kernel on one row (per-thread device buffers and stream; the host path spreads a batch over threads)
static double lisa_loglike(void*, const state& s) {
  struct Buf {
    double* x = nullptr;
    double* out = nullptr;
    hipStream_t st = nullptr;
    Buf() {
      if (hipMalloc((void**)&x, 6 * sizeof(double)) != hipSuccess || hipMalloc((void**)&out, sizeof(double)) != hipSuccess ||
          hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
        std::cout << "lisa_loglike: no device buffers" << std::endl;
        exit(1);
      }
    }
    ~Buf() { (void)hipFree(x); (void)hipFree(out); (void)hipStreamDestroy(st); }
  };
  static thread_local Buf b;
  const std::vector<double> x = s.get_params_vector();
  double r = 0;
  if (hipMemcpyAsync(b.x, x.data(), 6 * sizeof(double), hipMemcpyHostToDevice, b.st) != hipSuccess) exit(1);
  lisa_loglike_device(nullptr, (void*)b.st, 1, 6, b.x, nullptr, b.out);
  if (hipMemcpyAsync(&r, b.out, sizeof(double), hipMemcpyDeviceToHost, b.st) != hipSuccess || hipStreamSynchronize(b.st) != hipSuccess) exit(1);
  return r;
}

class lisa_device_like : public device_likelihood {
 public:
  void evaluate_log_device(void* stream, int n_rows, int dim, const double* X_dev, const int32_t* count_dev, double* out_dev) override {
    lisa_loglike_device(nullptr, stream, n_rows, dim, X_dev, count_dev, out_dev);
  }
};

// the likelihood's set-up (the reference's simple_likelihood_setup_nc, exampleLISA.cc:528-593, in this program's words)
static void setup_likelihood(bayes_likelihood* like) {
  const int D = 6;
  const double PI = M_PI;
  stateSpace space(D);
  space.set_names(std::vector<std::string>{"d", "phi", "inc", "lambda", "beta", "psi"});
  space.set_bound(0, boundary(boundary::limit, boundary::limit, 0, 30));
  space.set_bound(1, boundary(boundary::wrap, boundary::wrap, 0, 2 * PI));
  space.set_bound(2, boundary(boundary::limit, boundary::limit, 0, PI));
  space.set_bound(3, boundary(boundary::wrap, boundary::wrap, 0, 2 * PI));
  space.set_bound(4, boundary(boundary::limit, boundary::limit, -PI / 2, PI / 2));
  space.set_bound(5, boundary(boundary::wrap, boundary::wrap, 0, PI));
  like->register_evaluate_log(lisa_loglike);
  const std::vector<std::string> types = {"uni", "uni", "pol", "uni", "cpol", "uni"};
  const std::vector<double> centers = {1.667, PI, PI / 2, PI, 0, PI / 2}, scales = {1.333, PI, PI / 2, PI, PI / 2, PI / 2};
  like->basic_setup(&space, types, centers, scales);
}

int main(int argc, char* argv[]) {
  ptmcmc_sampler::Init(argc, argv);
  Options opt(true);
  // create the sampler
  ptmcmc_sampler mcmc;
  bayes_sampler* s0 = &mcmc;
  // create the likelihood
  bayes_likelihood* like = new lisa_device_like();
  setup_likelihood(like);

  // prep command-line options
  s0->addOptions(opt);
  like->addOptions(opt);
  opt.add(Option("nchains", "How many chains to run, one after the other. [1]", "1"));
  opt.add(Option("seed", "Seed of the random streams, a number in [0,1). [-1: seed from the clock]", "-1"));
  opt.add(Option("precision", "Significant digits in the chain files. [13]", "13"));
  opt.add(Option("outname", "Stem of the output file names. [mcmc_output]", "mcmc_output"));
  const bool parseBAD = opt.parse(argc, argv);
  if (parseBAD) {
    std::cout << "Usage:\n example_lisa_device [--options=vals] " << std::endl;
    std::cout << opt.print_usage() << std::endl;
    return 1;
  }
  std::cout << "flags=\n" << opt.report() << std::endl;
  like->setup();

  double seed;
  int Nchain, output_precision;
  std::string outname;
  std::istringstream(opt.value("nchains")) >> Nchain;
  std::istringstream(opt.value("seed")) >> seed;
  if (seed < 0) seed = std::fmod(time(NULL) / 3.0e7, 1);   // seed from the clock
  std::istringstream(opt.value("precision")) >> output_precision;
  std::istringstream(opt.value("outname")) >> outname;
  if (argc > 1) outname = argv[1];   // (a bare first argument names the output too)
  std::cout.precision(output_precision);
  std::cout << "\noutname = '" << outname << "'" << std::endl;
  std::cout << "seed=" << seed << std::endl;
  ProbabilityDist::setSeed(seed);

  // the space / prior, for the report
  const stateSpace space = *like->getObjectStateSpace();
  std::cout << "like.nativeSpace=\n" << space.show() << std::endl;
  std::shared_ptr<const sampleable_probability_function> prior = like->getObjectPrior();
  std::cout << "Prior is:\n" << prior->show() << std::endl;
  std::cout << "Npar=" << space.size() << std::endl;

  // Bayesian sampling: set up the sampler and its proposal distribution
  mcmc.setup(*like, output_precision);
  mcmc.select_proposal();

  const std::string base = outname;
  for (int ic = 0; ic < Nchain; ic++) {
    bayes_sampler* s = s0->clone();
    s->initialize();
    s->run(base, ic);
    ptmcmc_sampler* ps = dynamic_cast<ptmcmc_sampler*>(s);
    std::cout << ps->chains()->status();
    std::cout << "MAP: lpost = " << ps->chains()->getMAPlpost() << " at " << ps->chains()->getMAPstate().get_string() << std::endl;
    std::cout << "proposals drawn on the " << (ps->chains()->proposals_on_host() ? "host" : "device")
              << (ps->chains()->draws_de_on_device() ? " (differential evolution from the device's own history)" : "")
              << (ps->chains()->draws_prior_on_device() ? " (prior draws on the device; PTM_HOST_PRIOR_DRAW=1: the host path)" : "") << std::endl;
    delete s;
  }
  // summary
  std::cout << "best_post " << like->bestPost() << ", state=" << like->bestState().get_string() << std::endl;
  delete like;
  return 0;
}
