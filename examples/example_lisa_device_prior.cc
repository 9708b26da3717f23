// example_lisa_device_prior.cc -- examples/example_lisa_device.cc with a prior that is NOT a per-dimension product, also ON THE DEVICE:
// the same main(), call for call, but the prior is a device_prior (ptmcmc_gpu.hh) whose evaluate_log_prior_device launches the HIP
// kernel of examples/correlated_prior_device.hip on the engine's stream -- the toy-LISA product prior times a correlated Gaussian in
// distance and inclination, with a hard cut.  The step is then propose pass -> pack of the valid proposals -> the prior's kernel ->
// prior gate -> pack of the wanted proposals -> the likelihood's kernel -> scatter -> accept pass, with no host wait.  Without
// device_prior such a prior costs the whole device path: it goes through ptm_set_prior_callback and takes the likelihood to the host
// with it, which is what PTM_DEVICE_PRIOR=0 in the environment still does.  The prior's host evaluate_log is the kernel's own function
// compiled for the host (+ - * / and comparisons only: the same bits), so both routes write the same chains.
//   build: hipcc --offload-arch=gfx950 -std=c++17 -O2 -ffp-contract=off -Iinclude -Iptmcmc_amd/host examples/example_lisa_device_prior.cc examples/lisa_device_likelihood.hip examples/correlated_prior_device.hip -Lptmcmc_amd -lptm_engine -Wl,-rpath,$PWD/ptmcmc_amd -o lisa_device_prior
//   usage: as example_lisa; PTM_DEVICE_PRIOR=0 forces the host route
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
// examples/correlated_prior_device.hip
extern "C" void correlated_logprior_device(void* user, void* stream, int n_rows, int dim, const double* X_dev, const int32_t* count_dev,
                                           double* out_lprior_dev);
extern "C" double correlated_logprior_host(const double* x);

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

// the prior: evaluated by the kernel (device route) or by the kernel's function on the host (host route); drawn on the host by
// rejection from the product prior it is built on (the start states)
class correlated_prior : public device_prior {
  mixed_dist_product product;

 public:
  correlated_prior(const stateSpace* sp, const std::valarray<int>& types, const std::valarray<double>& centers, const std::valarray<double>& scales)
      : device_prior(sp), product(sp, types, centers, scales) { dim = 6; }
  void evaluate_log_prior_device(void* stream, int n_rows, int dim_, const double* X_dev, const int32_t* count_dev, double* out_dev) const override {
    correlated_logprior_device(nullptr, stream, n_rows, dim_, X_dev, count_dev, out_dev);
  }
  double evaluate_log(state& s) const override {
    if (s.invalid()) return -INFINITY;
    const std::vector<double> x = s.get_params_vector();
    return correlated_logprior_host(x.data());
  }
  double evaluate(state& s) const override { return std::exp(evaluate_log(s)); }
  // the product prior's draw, kept with the probability of the Gaussian factor (at most 1) inside the cut
  state drawSample(Random& rng) const override {
    for (;;) {
      state s = product.drawSample(rng);
      state probe = s;
      const double lp = evaluate_log(probe), lp0 = product.evaluate_log(probe);
      if (!(lp > -INFINITY)) continue;
      const double lg = lp - lp0;   // the Gaussian factor times a constant below 1 (LOG_NORM is less than the product prior's constant)
      if (std::log(rng.Next()) < lg) return s;
    }
  }
  void getScales(std::valarray<double>& out) const override { product.getScales(out); }
  std::string show() const override { return "CorrelatedPrior(MixedDistProduct(dim=6) x Gaussian(d, inc), d <= 2.6)"; }
};

// the likelihood's set-up (the reference's simple_likelihood_setup_nc, exampleLISA.cc:528-593, in this program's words), with the prior
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
  const std::valarray<int> types = {mixed_dist_product::uniform, mixed_dist_product::uniform, mixed_dist_product::polar,
                                    mixed_dist_product::uniform, mixed_dist_product::copolar, mixed_dist_product::uniform};
  const std::valarray<double> centers = {1.667, PI, PI / 2, PI, 0, PI / 2}, scales = {1.333, PI, PI / 2, PI, PI / 2, PI / 2};
  // (the likelihood copies the space: the prior lives on the copy)
  like->basic_setup(&space, new correlated_prior(like->getObjectStateSpace(), types, centers, scales));
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
    std::cout << "Usage:\n example_lisa_device_prior [--options=vals] " << std::endl;
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
              << (ps->chains()->draws_de_on_device() ? " (differential evolution from the device's own history)" : "") << std::endl;
    std::cout << "prior evaluated on the " << (ps->chains()->prior_evaluated_on_device() ? "device" : "host (PTM_DEVICE_PRIOR=0, or host-side proposals)") << std::endl;
    std::cout << "step kernel: " << ps->chains()->step_kernel_name() << std::endl;
    delete s;
  }
  // summary
  std::cout << "best_post " << like->bestPost() << ", state=" << like->bestState().get_string() << std::endl;
  delete like;
  return 0;
}
