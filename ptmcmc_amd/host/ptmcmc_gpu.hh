// ptmcmc_gpu.hh -- host-side C++ mirror of ptmcmc's plug-in surface for the chain::step() path, on top of the C ABI
// (include/ptm_engine.h).  Header only, C++11, no HIP types: link against libptm_engine.so.
//
// Same class names, constructor arguments and call sequence as the reference, so that user code written against
//   states.hh / probability_function.hh / proposal_distribution.hh / bayesian.hh / chain.hh / ptmcmc.hh
// reads the same here (namespace ptmgpu; `using namespace ptmgpu;` gives the reference's global names):
//
//   stateSpace space(D); space.set_bound(i, boundary(boundary::wrap, boundary::wrap, 0, 2*M_PI));      states.hh:29-145
//   bayes_likelihood like;  like.basic_setup(&space, types, centers, scales);                        bayesian.hh:360-381
//   like.register_reference_object(obj);  like.register_evaluate_log(fn);                            bayesian.hh:536-552
//   gaussian_prop prop(cov_or_sigmas, oneDfrac);                                       proposal_distribution.hh:145-227
//   parallel_tempering_chains ptc(Ntemps, Tmax, swap_rate, add_every_N);                                chain.cc:1163
//   ptc.initialize(&like, like.getObjectPrior().get(), 1);  ptc.set_proposal(prop);                  chain.cc:1281,1367
//   for (...) ptc.step();                                                                               chain.cc:1393
//   ptc.subchain(i)->getState() / getLogPost() / getLogLike() / invTemp()                             chain.hh:89-141
//
// What runs where: these classes only DESCRIBE the problem (bounds, per-dimension prior, target, ladder, per-rung
// proposal factor) to the engine; every step() is kernels on the MI355X.  A likelihood registered as a function pointer is
// called on the host between the propose and the accept kernel (batched); `gaussian_likelihood` is evaluated on the
// device.  Errors follow the reference: print and exit(1) (chain.cc:967-971, states.cc:87-90).
#ifndef PTMCMC_GPU_HH
#define PTMCMC_GPU_HH

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <valarray>
#include <vector>
#include <sched.h>
#include <sys/stat.h>
#include <sys/types.h>

#include "ptm_engine.h"

namespace ptmgpu {

inline void ptm_check(int rc, const char* what) {
  if (rc != PTM_OK) {
    std::cout << what << ": " << ptm_last_error() << std::endl;
    exit(1);
  }
}

// what must happen to an engine of the facade before it is destroyed: a device likelihood keeps the engine's best evaluated posterior
// (the engine holds it on the device) -- the hooks are registered by device_likelihood and removed by its destructor
inline std::map<ptm_engine*, std::function<void(ptm_engine*)>>& engine_release_hooks() { static std::map<ptm_engine*, std::function<void(ptm_engine*)>> m; return m; }
inline std::mutex& engine_hooks_mutex() { static std::mutex m; return m; }
inline void engine_gone(ptm_engine* e) {
  std::function<void(ptm_engine*)> f;
  {
    std::lock_guard<std::mutex> lk(engine_hooks_mutex());
    auto it = engine_release_hooks().find(e);
    if (it == engine_release_hooks().end()) return;
    f = it->second;
    engine_release_hooks().erase(it);
  }
  f(e);
}

// ---- states.hh --------------------------------------------------------------------------------------------------
class boundary {  // states.hh:29-48
  int lowertype, uppertype;
  double xmin, xmax;

 public:
  static const int open = 0, limit = 1, reflect = 2, wrap = 3;
  boundary(int lowertype = open, int uppertype = open, double min = -INFINITY, double max = INFINITY)
      : lowertype(lowertype), uppertype(uppertype), xmin(min), xmax(max) {}
  void getDomainLimits(double& xmin_, double& xmax_) const { xmin_ = xmin; xmax_ = xmax; }
  bool isWrapped() const { return lowertype == wrap && uppertype == wrap; }
  // boundary::enforce (states.cc:11-58), on the host for states the HOST builds (proposals drawn on the host side); the
  // device enforces every proposal again with the same rules (ptm_kernels.hpp boundary_enforce)
  bool enforce(double& x) const {
    if ((lowertype == wrap) != (uppertype == wrap)) return false;
    if (lowertype == wrap) {
      const double width = xmax - xmin;
      if (width <= 0) return false;
      double xt = std::fmod(x - xmin, width);
      if (xt < 0) xt += width;
      x = xmin + xt;
      return true;
    }
    if (lowertype == reflect && uppertype == reflect) {
      const double halfwidth = xmax - xmin;
      if (halfwidth <= 0) return false;
      const double width = 2 * halfwidth;
      double xt = std::fmod(x - xmin, width);
      if (xt < 0) xt += width;
      if (xt >= halfwidth) xt = halfwidth - xt;   // as the reference folds it (states.cc:41)
      x = xmin + xt;
      return true;
    }
    if (lowertype == reflect && x < xmin) x = xmin + (xmin - x);
    else if (uppertype == reflect && x > xmax) x = xmax - (x - xmax);
    if (lowertype == limit && x < xmin) return false;
    if (uppertype == limit && x > xmax) return false;
    return true;
  }
  int lower() const { return lowertype; }
  int upper() const { return uppertype; }
  std::string show() const {
    std::ostringstream s;
    if (lowertype == wrap) s << "w[" << xmin << "," << xmax << ")w";
    else s << (lowertype == reflect ? "R[" : lowertype == limit ? "[" : "(") << xmin << "," << xmax
           << (uppertype == reflect ? "]R" : uppertype == limit ? "]" : ")");
    return s.str();
  }
};

class stateSpace {  // states.hh:60-145 (names, bounds; symmetries are out of scope)
  int dim;
  std::vector<boundary> bounds;
  std::vector<std::string> names;
  std::map<std::string, int> index;
  bool have_names;

 public:
  stateSpace(int dim = 0) : dim(dim), bounds(dim), have_names(false) {}
  int size() const { return dim; }
  void set_bound(int i, const boundary& b) {
    if (i < dim) bounds[i] = b;
    else { std::cout << "stateSpace::set_bound: Index out of range, " << i << ">=" << dim << "." << std::endl; exit(1); }
  }
  boundary get_bound(int i) const {
    if (i < 0 || i >= dim) { std::cout << "stateSpace::set_bound: Index out of range, " << i << ">=" << dim << "." << std::endl; exit(1); }
    return bounds[i];
  }
  void set_names(const std::vector<std::string>& n) {
    if ((int)n.size() < dim) { std::cout << "stateSpace::set_names: Vector of param names is too short. Quitting." << std::endl; exit(-1); }
    names.assign(n.begin(), n.begin() + dim);
    for (int i = 0; i < dim; i++) index[names[i]] = i;
    have_names = true;
  }
  void set_names(const std::string n[]) { set_names(std::vector<std::string>(n, n + dim)); }
  std::string get_name(int i) const { return have_names && i < dim ? names[i] : "[unnamed]"; }
  bool enforce(std::valarray<double>& params) const {   // states.cc:86-102
    if ((int)params.size() != dim) { std::cout << "stateSpace::enforce:  Dimension error.  Expected " << dim << " params, but given " << params.size() << "." << std::endl; exit(1); }
    for (int i = 0; i < dim; i++)
      if (!bounds[i].enforce(params[i])) return false;
    return true;
  }
  int get_index(const std::string& name) const { return have_names && index.count(name) ? index.at(name) : -1; }
  int requireIndex(const std::string& name) const {
    int i = get_index(name);
    if (i < 0) { std::cout << "stateSpace::checkNames(): Name '" << name << "' not found in state space." << std::endl; exit(1); }
    return i;
  }
  std::string show() const {
    std::ostringstream s;
    s << "StateSpace:(dim=" << dim << ")\n";
    for (int i = 0; i < dim; i++) s << "  " << get_name(i) << " in " << bounds[i].show() << "\n";
    return s.str();
  }
};

class state {  // states.hh:147-234, states.cc:161-253
  const stateSpace* space;
  std::valarray<double> params;
  bool valid;

 public:
  // state(space, n): the zero vector, ENFORCED (states.cc:168-176) -- quirk Q9: if zero violates a `limit` bound the state is
  // born invalid, and every state::add() result with it
  state(const stateSpace* space = nullptr, int n = 0) : space(space), params(0.0, n), valid(space != nullptr) { if (space) enforce(); }
  state(const stateSpace* sp, const std::valarray<double>& a) : space(sp), params(a), valid(sp != nullptr) { enforce(); }
  state(const stateSpace* sp, const std::vector<double>& a) : space(sp), params(a.data(), a.size()), valid(sp != nullptr) { enforce(); }
  // values the engine hands back: enforced on the device already
  static state from_engine(const stateSpace* sp, const double* x, int n) { state s; s.space = sp; s.params = std::valarray<double>(x, n); s.valid = sp != nullptr; return s; }
  void enforce() {   // states.cc:161-166
    if (!space) valid = false;
    if (!valid) return;
    valid = space->enforce(params);
  }
  int size() const { return params.size(); }
  double get_param(int i) const { return params[i]; }
  double get_param(const std::string& name) const { return params[space->requireIndex(name)]; }
  void set_param(int i, double v) { params[i] = v; }
  std::valarray<double> get_params() const { return params; }
  std::vector<double> get_params_vector() const { return std::vector<double>(std::begin(params), std::end(params)); }
  const stateSpace* getSpace() const { return space; }
  bool invalid() const { return !valid; }
  // The state a chain of state::scalar_mult / state::add operations starting from this one ends in (states.cc:183-214): those
  // build on the ENFORCED ORIGIN of the space -- valid iff the origin is (quirk Q9) -- and do not enforce their result.
  state moved_to(const std::vector<double>& x) const {
    state r(space, size());
    for (int i = 0; i < size() && i < (int)x.size(); i++) r.params[i] = x[i];
    return r;
  }
  // the vector-space operations some proposals rely on (states.cc:194-253; extra_enforcement is off in the reference)
  state add(const state& other) const {
    state result(space, size());
    if (other.size() != size()) { std::cout << "state::add: Sizes mismatch. (" << size() << "!=" << other.size() << ")\n"; exit(1); }
    for (int i = 0; i < size(); i++) result.params[i] = params[i] + other.params[i];
    return result;
  }
  state scalar_mult(double x) const {
    state result(space, size());
    for (int i = 0; i < size(); i++) result.params[i] = params[i] * x;
    return result;
  }
  double innerprod(const state& other, bool constrained = false) const {
    if (constrained && !(valid && other.valid)) return NAN;
    if (other.size() != size()) { std::cout << "state::innerprod: sizes mismatch.\n"; exit(1); }
    double result = 0;
    for (int i = 0; i < size(); i++) result += params[i] * other.params[i];
    return result;
  }
  std::vector<int> projection_indices_by_name(const stateSpace* subspace) const {   // states.cc:256-264
    std::vector<int> idx;
    for (int isub = 0; isub < subspace->size(); isub++) idx.push_back(space ? space->get_index(subspace->get_name(isub)) : -1);
    return idx;
  }
  std::string get_string(int prec = -1) const {
    std::ostringstream s;
    if (prec > 0) s.precision(prec);
    for (int i = 0; i < size(); i++) s << (i ? ", " : "") << params[i];
    return s.str();
  }
};

// ---- ProbabilityDist / newran: what the plug-in surface sees of the random numbers ----------------------------------------
// The reference hands every chain its own newran generator and proposals pull uniforms with caller->getPRNG()->Next()
// (chain.hh:44-75).  Here a chain's host-side generator is one more counter-based Philox4x32-10 stream -- keyed like the
// device streams by (seed, walker, rung, step), in a tag domain of its own -- so host-side proposals are as reproducible and
// as independent of the launch geometry as the device's.
class Random {
 public:
  virtual ~Random() {}
  virtual double Next() = 0;   // uniform in (0, 1)
};

namespace detail {
inline void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {   // Salmon et al., SC'11
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
}  // namespace detail

class philox_random : public Random {   // counter: (block, stream, step[31:0], step[55:32] | tag << 24), tag 3 = host proposals
  uint64_t seed, step;
  uint32_t stream, block, buf[4];
  int have;

 public:
  philox_random() : seed(0), step(0), stream(0), block(0), have(0) {}
  void reseat(uint64_t seed_, uint32_t stream_, uint64_t step_) { seed = seed_; stream = stream_; step = step_; block = 0; have = 0; }
  double Next() override {
    if (!have) {
      const uint32_t ctr[4] = {block++, stream, (uint32_t)step, ((uint32_t)(step >> 32) & 0x00FFFFFFu) | (3u << 24)};
      const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
      detail::philox4x32_10(ctr, key, buf);
      have = 4;
    }
    return ((double)buf[4 - have--] + 0.5) * (1.0 / 4294967296.0);   // newran's open-interval map (newran1.cxx:432)
  }
  // a standard normal (Box-Muller on two uniforms; the device has its own table-driven form for its own draws)
  double Normal() {
    const double u1 = Next(), u2 = Next();
    return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
  }
};

class ProbabilityDist {   // ProbabilityDist.h:37-48: the master seed every chain's generator descends from
 public:
  static double& seed_ref() { static double s = -1; return s; }
  static void setSeed(double seed) { seed_ref() = seed; }
  static double getSeed() { return seed_ref(); }
  // the engine's Philox key for a seed in [0, 1) (< 0: the fixed default)
  static uint64_t engineSeed() { const double s = seed_ref(); return s >= 0 ? (uint64_t)(s * 4294967296.0) : 0x5EED0001ull; }
  // The reference seeds every chain from the master generator in construction order (chain.hh:58-62), so the ladders a
  // program builds one after the other (its loop over clone() / initialize() / run()) differ.  Here: the n-th ladder of the
  // process gets the master key with n folded into the upper word (the first one the master key itself).
  static int& ladders_made() { static int n = 0; return n; }
  static uint64_t nextLadderSeed() { const uint64_t n = (uint64_t)ladders_made()++; return engineSeed() ^ (n * 0x9E3779B97F4A7C15ull << 32); }
};

// ---- command-line flags ("--name=value", bare "--name" = "true") ------------------------------------------------------------
// The reference's programs declare their flags through three small classes (options.hh): every component registers
// Option(name, help, default) objects in one shared Options table (Optioned::addOptions / addOption), main() adds its own and
// calls Options::parse(argc, argv), and the components read their values back by name (optValue / optSet).  Only that calling
// surface -- the class and method names and the flag syntax -- is kept; the table below is this build's own: entries in one
// vector in order of declaration, a name index beside it, and argv compacted in a single pass.
class Options;
class Option {
  friend class Options;
  enum origin { none, preset, command_line };
  std::string key, help, text;
  origin from;

 public:
  Option() : from(none) {}
  Option(const std::string& name, const std::string& info, const std::string& vdefault = "<no default>")
      : key(name), help(info), text(vdefault == "<no default>" ? std::string() : vdefault), from(vdefault == "<no default>" ? none : preset) {}
  // one line that identifies the declaration (two declarations of a flag must agree in it)
  std::string describe() const { return key + "('" + help + "')=" + (from == none ? std::string("<no value>") : text); }
};

class Options {
  std::vector<Option> table;
  std::map<std::string, size_t> where;
  std::string lead;   // "--" or "-"

  const Option* find(const std::string& name) const {
    std::map<std::string, size_t>::const_iterator it = where.find(name);
    return it == where.end() ? nullptr : &table[it->second];
  }
  // is `word` a flag of this table's syntax?  If so its name and, after '=', its value ("true" for a bare flag)
  bool as_flag(const std::string& word, std::string& name, std::string& val) const {
    if (word.size() <= lead.size() || word.compare(0, lead.size(), lead) != 0) return false;
    const size_t eq = word.find('=', lead.size());
    name = word.substr(lead.size(), eq == std::string::npos ? std::string::npos : eq - lead.size());
    val = eq == std::string::npos ? std::string("true") : word.substr(eq + 1);
    return true;
  }
  // records a recognised flag; false (and a complaint, if wanted) for one nobody declared
  bool take(const std::string& name, const std::string& val, bool verbose) {
    std::map<std::string, size_t>::iterator it = where.find(name);
    if (it == where.end()) {
      if (verbose) std::cerr << "Option '" << name << "' not recognized." << std::endl;
      return false;
    }
    table[it->second].text = val;
    table[it->second].from = Option::command_line;
    return true;
  }

 public:
  Options(bool dash_dash = true) : lead(dash_dash ? "--" : "-") {}
  void add(const Option& opt) {
    if (const Option* have = find(opt.key)) {   // the first declaration stands; a different second one is worth a warning
      if (have->describe() != opt.describe())
        std::cout << "Options::add: flag '" << opt.key << "' is declared twice with different help / default; keeping " << have->describe() << std::endl;
      return;
    }
    where[opt.key] = table.size();
    table.push_back(opt);
  }
  bool exists(const std::string& name) const { return find(name) != nullptr; }
  // true if the flag has a value (given, or a default); the value goes to return_value
  bool set(const std::string& name, std::string& return_value) const {
    const Option* o = find(name);
    if (!o) { std::cerr << "Options: Error no option '" << name << "'." << std::endl; return false; }
    if (o->from == Option::none) return false;
    return_value = o->text;
    return true;
  }
  bool set(const std::string& name) const { std::string unused; return set(name, unused); }
  std::string value(const std::string& name) const { std::string v; set(name, v); return v; }
  std::string print_usage() const {
    std::ostringstream os;
    os << "Options:\n";
    for (std::map<std::string, size_t>::const_iterator it = where.begin(); it != where.end(); ++it) {   // by name
      std::string head = "  " + lead + it->first;
      if (head.size() < 26) head.resize(26, ' ');
      os << head << "  " << table[it->second].help << "\n";
    }
    return os.str();
  }
  // Flags this table knows are recorded and taken out of argv (argc shrinks); every other word stays where it is, in order.
  // Returns true if some word looked like a flag but was not declared (the caller may have a second table for those).
  bool parse(int& argc, char* argv[], bool verbose = true) {
    bool unknown = false;
    int kept = argc > 0 ? 1 : 0;
    for (int i = kept; i < argc; i++) {
      std::string name, val;
      if (as_flag(argv[i], name, val)) {
        if (take(name, val, verbose)) continue;
        unknown = true;
      }
      argv[kept++] = argv[i];
    }
    argc = kept;
    return unknown;
  }
  // the same on a vector of words that does not start with the program name
  bool parse(std::vector<std::string>& words, bool verbose = true) {
    bool unknown = false;
    std::vector<std::string> rest;
    for (size_t i = 0; i < words.size(); i++) {
      std::string name, val;
      if (as_flag(words[i], name, val)) {
        if (take(name, val, verbose)) continue;
        unknown = true;
      }
      rest.push_back(words[i]);
    }
    words.swap(rest);
    return unknown;
  }
  std::string report() const {
    std::ostringstream s;
    for (std::map<std::string, size_t>::const_iterator it = where.begin(); it != where.end(); ++it) {
      const Option& o = table[it->second];
      s << " " << it->first << ':' << (o.from == Option::command_line ? o.text : std::string("(not set)")) << '\n';
    }
    return s.str();
  }
};

// mix-in of every component that declares flags: addOptions(table, prefix) binds it to the program's table, addOption declares,
// optValue / optGetValue / optSet read back
class Optioned {
  Options* bound;
  std::string scope;   // prefix of this component's flag names

  Options& options() const {
    if (!bound) { std::cout << "Optioned: addOptions() has not been called for this object; it has no flags to read." << std::endl; exit(1); }
    return *bound;
  }

 protected:
  void copyOptioned(const Optioned& other) { bound = other.bound; scope = other.scope; }
  void addOption(const std::string& name, const std::string& info, const std::string& vdefault = "<no default>") { options().add(Option(scope + name, info, vdefault)); }

 public:
  Optioned() : bound(nullptr) {}
  virtual ~Optioned() {}
  virtual void addOptions(Options& opts, const std::string& prefix_ = "") { bound = &opts; scope = prefix_; }
  bool haveOptions() const { return bound != nullptr; }
  std::unique_ptr<std::istringstream> optValue(const std::string& name) { return std::unique_ptr<std::istringstream>(new std::istringstream(options().value(scope + name))); }
  template <class T> void optGetValue(const std::string& name, T& val) { *optValue(name) >> val; }
  bool optSet(const std::string& name) { return options().set(scope + name); }
  std::string reportOptions() { return options().report(); }
};

// ---- probability_function.hh --------------------------------------------------------------------------------------
class probability_function {  // probability_function.hh:31-44
 protected:
  const stateSpace* space;

 public:
  virtual ~probability_function() {}
  probability_function(const stateSpace* space) : space(space) {}
  virtual double evaluate_log(state& s) { return 0; }
  const stateSpace* get_space() const { return space; }
};

class sampleable_probability_function : public probability_function {  // probability_function.hh:48-83
 protected:
  unsigned int dim;

 public:
  sampleable_probability_function(const stateSpace* space) : probability_function(space), dim(0) {}
  virtual int getDim() const { return dim; }
  virtual void getScales(std::valarray<double>& out) const {}
  virtual void getScales(std::vector<double>& out) const { std::valarray<double> v; getScales(v); out.assign(std::begin(v), std::end(v)); }
  // host-side evaluation and sampling (probability_function.hh:48-83), for proposals that draw from the prior and for the
  // likelihood's best-posterior bookkeeping; the chain's own prior values are computed on the device
  virtual double evaluate(state& s) const { return 1; }
  virtual double evaluate_log(state& s) const { return std::log(evaluate(s)); }   // probability_function.hh:59
  virtual state drawSample(Random& rng) const { std::cout << "sampleable_probability_function::drawSample: not defined for this prior" << std::endl; exit(1); }
  virtual std::string show() const { return "UnspecifiedSampleableProbabilityFunction()"; }
  // engine description: per-dimension (type, center, halfwidth), types as mixed_dist_product::{uniform,...}; true if the prior
  // IS such a product -- it is then evaluated and drawn from on the device.  Any other prior (false, the default: a subclass
  // need only give evaluate / evaluate_log and drawSample, as in the reference) is evaluated on the host, through the engine's
  // prior callback (ptm_set_prior_callback), and the chains' start states are drawn with its drawSample.
  virtual bool describe(std::vector<int>& types, std::vector<double>& centers, std::vector<double>& halfwidths) const { return false; }
};

// A prior that is not a per-dimension product, evaluated ON THE DEVICE (ptm_set_prior_device) beside a device_likelihood: the engine
// calls evaluate_log_prior_device once per sweep on its own stream with the VALID proposals in device memory (X_dev [n_rows][dim], rows
// [0, *count_dev) to evaluate, the rest in-support states); it enqueues its work on `stream` (a hipStream_t) and returns; -inf = outside
// the support.  The host evaluate_log and drawSample stay required: the start states are drawn on the host, and the ladder keeps the
// host path (ptm_set_prior_callback) when the likelihood is no device_likelihood, with host-side proposals, or with PTM_DEVICE_PRIOR=0
// in the environment.  Host and device must give the same bits for the two paths to walk the same chains.
class device_prior : public sampleable_probability_function {
 public:
  device_prior(const stateSpace* space) : sampleable_probability_function(space) {}
  virtual void evaluate_log_prior_device(void* stream, int n_rows, int dim, const double* X_dev, const int32_t* count_dev, double* out_dev) const = 0;
  static void device_trampoline(void* self, void* stream, int n_rows, int dim, const double* X_dev, const int32_t* count_dev, double* out_dev) {
    ((const device_prior*)self)->evaluate_log_prior_device(stream, n_rows, dim, X_dev, count_dev, out_dev);
  }
  static bool wanted() {
    const char* v = getenv("PTM_DEVICE_PRIOR");
    return !(v && *v == '0');
  }
};

class mixed_dist_product : public sampleable_probability_function {  // probability_function.hh:141-170, .cc:219-262
 protected:
  std::valarray<int> types;
  std::valarray<double> centers, halfwidths;

 public:
  static const int uniform = 1, gaussian = 2, polar = 3, copolar = 4, log = 5;
  mixed_dist_product(const stateSpace* space, const std::valarray<int>& types, const std::valarray<double>& centers,
                     const std::valarray<double>& halfwidths)
      : sampleable_probability_function(space), types(types), centers(centers), halfwidths(halfwidths) {
    dim = centers.size();
    if (dim != halfwidths.size() || dim != types.size() || (space && (unsigned)space->size() > dim)) {
      std::cout << "mixed_dist_product(constructor): Array sizes mismatch.\n";
      exit(1);
    }
    for (unsigned i = 0; i < dim; i++)
      if (types[i] == log && (centers[i] <= 0 || halfwidths[i] <= 1)) {
        std::cout << "mixed_dist_product(constructor): Need centers>0 and halfwidths>1 for log-type dimension [" << i << "]." << std::endl;
        exit(1);
      }
  }
  void getScales(std::valarray<double>& out) const override { out = halfwidths; }
  // mixed_dist_product::evaluate (probability_function.cc:281-304): the product of the 1-D pdfs of ProbabilityDist.h:76-257;
  // an invalid state has probability 0
  double evaluate(state& s) const override {
    if (s.invalid()) return 0;
    double result = 1;
    for (unsigned i = 0; i < dim; i++) result *= pdf1(i, s.get_param(i));
    return result;
  }
  // ... and its drawSample (probability_function.cc:264-279): one draw per dimension from the 1-D distribution's inverse cdf
  // (uniform / log / polar / copolar) or a normal (gaussian)
  state drawSample(Random& rng) const override {
    std::valarray<double> x(dim);
    for (unsigned i = 0; i < dim; i++) {
      const double c = centers[i], h = halfwidths[i];
      switch (types[i]) {
        case uniform: x[i] = rng.Next() * (2 * h) + (c - h); break;
        case gaussian: { const double u1 = rng.Next(), u2 = rng.Next(); x[i] = std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2) * h + c; break; }
        case polar: { double a = c - h, b = c + h; if (a < 0) a = 0; if (b > M_PI) b = M_PI; const double ca = std::cos(a), cb = std::cos(b); x[i] = std::acos(ca - rng.Next() * (ca - cb)); break; }
        case copolar: { double a = c - h, b = c + h; if (a < -M_PI / 2) a = -M_PI / 2; if (b > M_PI / 2) b = M_PI / 2; const double sa = std::sin(a), sb = std::sin(b); x[i] = std::asin(sa + rng.Next() * (sb - sa)); break; }
        case log: { const double l0 = std::log(c / h), l1 = std::log(c * h); x[i] = std::exp(rng.Next() * (l1 - l0) + l0); break; }
        default: x[i] = NAN;
      }
    }
    return state(space, x);
  }
  std::string show() const override {
    std::ostringstream ss;
    ss << "MixedDistProduct(dim=" << dim << ")";
    return ss.str();
  }
  double pdf1(unsigned i, double x) const {
    const double c = centers[i], h = halfwidths[i];
    switch (types[i]) {
      case uniform: return (x < c - h || x > c + h) ? 0 : 1 / (2 * h);
      case gaussian: { const double xn = (x - c) / h; return std::exp(-xn * xn / 2) / std::sqrt(2 * M_PI) / h; }
      case polar: { double a = c - h, b = c + h; if (x < a || x > b) return 0; if (a < 0) a = 0; if (b > M_PI) b = M_PI; return std::sin(x) / (-std::cos(b) + std::cos(a)); }
      case copolar: { double a = c - h, b = c + h; if (x < a || x > b) return 0; if (a < -M_PI / 2) a = -M_PI / 2; if (b > M_PI / 2) b = M_PI / 2; return std::cos(x) / (std::sin(b) - std::sin(a)); }
      case log: { const double a = c / h, b = c * h; if (x < a || x > b) return 0; return 1 / (std::log(b) - std::log(a)) / x; }
    }
    return NAN;
  }
  bool describe(std::vector<int>& t, std::vector<double>& c, std::vector<double>& h) const override {
    t.assign(std::begin(types), std::end(types));
    c.assign(std::begin(centers), std::end(centers));
    h.assign(std::begin(halfwidths), std::end(halfwidths));
    return true;
  }
};

class uniform_dist_product : public mixed_dist_product {  // probability_function.hh:113-125
  static std::valarray<double> mid(const std::valarray<double>& a, const std::valarray<double>& b) { return (a + b) / 2.0; }
  static std::valarray<double> half(const std::valarray<double>& a, const std::valarray<double>& b) { return (b - a) / 2.0; }

 public:
  uniform_dist_product(const stateSpace* space, const std::valarray<double>& min_corner, const std::valarray<double>& max_corner)
      : mixed_dist_product(space, std::valarray<int>(uniform, min_corner.size()), mid(min_corner, max_corner), half(min_corner, max_corner)) {}
};

class gaussian_dist_product : public mixed_dist_product {  // probability_function.hh:92-108
 public:
  gaussian_dist_product(const stateSpace* space, const std::valarray<double>& x0s, const std::valarray<double>& sigmas)
      : mixed_dist_product(space, std::valarray<int>(gaussian, x0s.size()), x0s, sigmas) {}
};

// A prior on a direct product of independent state spaces (probability_function.hh:181-215, .cc:346-452): the product-space
// parameters are matched to the subspaces BY NAME; evaluate() is the product of the subspace priors on the projected states,
// drawSample() the direct product of subspace samples.  As in the reference the j-th parameter handed to subspace k is the
// j-th product-space parameter found in it, in PRODUCT-space order (.cc:387-405,443-447) -- name the subspaces' parameters in the
// order the product space lists them.  If every factor is a per-dimension product the whole is one and lives on the device.
class independent_dist_product : public sampleable_probability_function {
  std::vector<const sampleable_probability_function*> ss_dists;
  std::vector<const stateSpace*> ss;
  std::vector<int> index_ss, index_ss_index;      // product index -> subspace, index within it
  std::vector<std::vector<int> > ss_indices;      // subspace -> product indices found in it, in product order

 public:
  independent_dist_product(const stateSpace* product_space, const std::vector<const sampleable_probability_function*>& subspace_dists)
      : sampleable_probability_function(product_space) {
    dim = product_space->size();
    int dim_count = 0;
    for (size_t i = 0; i < subspace_dists.size(); i++)
      if (subspace_dists[i]->getDim() > 0) {   // empty subspaces are skipped
        ss_dists.push_back(subspace_dists[i]);
        ss.push_back(subspace_dists[i]->get_space());
        dim_count += subspace_dists[i]->getDim();
      }
    if ((int)dim != dim_count) {
      std::cout << "independent_dist_product(constructor): Total dimension of subspaces does not match product space dimension:" << std::endl;
      exit(1);
    }
    ss_indices.resize(ss.size());
    index_ss.resize(dim); index_ss_index.resize(dim);
    for (unsigned i = 0; i < dim; i++) {
      const std::string name = product_space->get_name(i);
      bool found = false;
      for (size_t j = 0; j < ss.size(); j++) {
        const int idx = ss[j]->get_index(name);
        if (idx < 0) continue;
        if (found) { std::cout << "independent_dist_product(constructor): Found name '" << name << "' in multiple spaces." << std::endl; exit(1); }
        found = true;
        index_ss[i] = (int)j; index_ss_index[i] = idx;
        ss_indices[j].push_back((int)i);
      }
      if (!found) { std::cout << "independent_dist_product(constructor): Did not find name '" << name << "' among subspace names." << std::endl; exit(1); }
    }
  }
  independent_dist_product(const stateSpace* product_space, const sampleable_probability_function* d1, const sampleable_probability_function* d2)
      : independent_dist_product(product_space, std::vector<const sampleable_probability_function*>{d1, d2}) {}
  independent_dist_product(const stateSpace* product_space, const sampleable_probability_function* d1, const sampleable_probability_function* d2,
                           const sampleable_probability_function* d3)
      : independent_dist_product(product_space, std::vector<const sampleable_probability_function*>{d1, d2, d3}) {}
  independent_dist_product(const stateSpace* product_space, const sampleable_probability_function* d1, const sampleable_probability_function* d2,
                           const sampleable_probability_function* d3, const sampleable_probability_function* d4)
      : independent_dist_product(product_space, std::vector<const sampleable_probability_function*>{d1, d2, d3, d4}) {}
  state drawSample(Random& rng) const override {
    std::vector<state> sub;
    for (size_t k = 0; k < ss.size(); k++) sub.push_back(ss_dists[k]->drawSample(rng));
    std::valarray<double> v(dim);
    for (unsigned i = 0; i < dim; i++) v[i] = sub[index_ss[i]].get_param(index_ss_index[i]);
    return state(space, v);
  }
  double evaluate(state& s) const override {
    if (s.invalid()) return 0;
    if ((int)dim != s.size()) { std::cout << "independent_dist_product:evaluate: State size mismatch.\n"; exit(1); }
    double result = 1;
    for (size_t k = 0; k < ss.size(); k++) {
      std::valarray<double> v(ss[k]->size());
      for (int j = 0; j < ss[k]->size(); j++) v[j] = s.get_param(ss_indices[k][j]);
      state sub(ss[k], v);
      result *= ss_dists[k]->evaluate(sub);
    }
    return result;
  }
  void getScales(std::valarray<double>& out) const override {
    out.resize(dim);
    int count = 0;
    for (size_t k = 0; k < ss.size(); k++) {
      std::valarray<double> sc;
      ss_dists[k]->getScales(sc);
      for (size_t j = 0; j < sc.size(); j++) out[count++] = sc[j];
    }
  }
  std::string show() const override {
    std::ostringstream o;
    o << "IndependentDistProduct(";
    for (size_t k = 0; k < ss.size(); k++) o << (k ? ", " : "") << ss_dists[k]->show();
    o << ")";
    return o.str();
  }
  bool describe(std::vector<int>& t, std::vector<double>& c, std::vector<double>& h) const override {
    t.assign(dim, 0); c.assign(dim, 0.0); h.assign(dim, 0.0);
    for (size_t k = 0; k < ss.size(); k++) {
      std::vector<int> tk;
      std::vector<double> ck, hk;
      if (!ss_dists[k]->describe(tk, ck, hk)) return false;
      for (size_t j = 0; j < tk.size() && j < ss_indices[k].size(); j++) {
        t[ss_indices[k][j]] = tk[j]; c[ss_indices[k][j]] = ck[j]; h[ss_indices[k][j]] = hk[j];
      }
    }
    return true;
  }
};

// ---- chain.hh: the base interface (what proposals and the driver see of a chain) -------------------------------------------
class proposal_distribution;
class chain {  // chain.hh:34-141
 public:
  virtual ~chain() {}
  virtual void step() = 0;
  virtual state getState(int elem = -1, bool raw_indexing = false) = 0;
  virtual double getLogPost(int elem = -1, bool raw_indexing = false) = 0;
  virtual double getLogLike(int elem = -1, bool raw_indexing = false) = 0;
  virtual double invTemp() { return 1.0; }
  virtual int multiplicity() { return 1; }
  virtual chain* subchain(int index) { return this; }
  virtual int getStep() = 0;
  virtual int size() { return getStep() + 1; }                       // saved history rows (chain.hh:86)
  virtual int getDim() { return 0; }
  virtual int get_id() { return 0; }
  virtual std::shared_ptr<Random> getPRNG() { return std::shared_ptr<Random>(); }   // chain.hh:75
  virtual double getMAPlpost() { return -1e200; }                    // chain.hh:116-117
  virtual state getMAPstate() { return getState(); }
  virtual std::string status() { return ""; }
  virtual std::string report_prop(int style = 0) { return ""; }
};

// ---- proposal_distribution.hh ---------------------------------------------------------------------------------------
// The whole plug-in surface of proposal_distribution.hh:38-88: draw(state&, chain*), log_hastings_ratio(), type(), accept() /
// reject(), clone(), set_chain(), is_ready(), support_mixing().  A proposal that can describe itself as a Gaussian with a fixed
// factor (device_describe) is drawn ON the device, fused into the sweep kernel; every other proposal -- differential
// evolution, sets of mixed members, user proposals with callbacks -- runs through the engine's host-proposal step
// (ptm_set_proposal_callback): draw() is called here, once per moving chain and step, and the device does the rest of
// MH_chain::step (enforce, prior, likelihood, Metropolis test).
class proposal_distribution {
 protected:
  int id;
  double log_hastings;
  int last_type, accept_count, reject_count;
  chain* ch;
  void* user_parent_object;
  void* user_instance_object;
  void* (*new_user_instance_object_function)(void* object, int id);
  static int& idcount() { static int n = 0; return n; }
  void set_instance() {   // proposal_distribution.hh:49-56
    if (user_parent_object && new_user_instance_object_function) user_instance_object = new_user_instance_object_function(user_parent_object, id);
    else user_instance_object = nullptr;
  }

 public:
  virtual ~proposal_distribution() {}
  proposal_distribution(void* user_parent_object = nullptr, void* (*new_user_instance_object_function)(void* object, int id) = nullptr)
      : log_hastings(0), last_type(0), accept_count(0), reject_count(0), ch(nullptr), user_parent_object(user_parent_object),
        user_instance_object(nullptr), new_user_instance_object_function(new_user_instance_object_function) {
    id = idcount()++;
    set_instance();
  }
  virtual double log_hastings_ratio() { return log_hastings; }   // proposal part of the Hastings ratio of the most recent draw
  virtual void set_chain(chain* c) { ch = c; }
  virtual state draw(state& s, chain* caller) { return s; }      // the base class is not useful
  virtual bool is_ready() { return true; }
  virtual proposal_distribution* clone() const { return new proposal_distribution(*this); }
  virtual std::string show() { return "UnspecifiedProposal()"; }
  virtual int type() { return last_type; }
  virtual bool support_mixing() { return false; }
  virtual void accept() { accept_count++; }
  virtual void reject() { reject_count++; }
  virtual void accept(int count) { accept_count = count; }
  virtual void reject(int count) { reject_count = count; }
  virtual void checkpoint(std::string path) {}
  virtual void restart(std::string path) {}
  virtual std::string report(int style = 0) {
    std::ostringstream ss;
    if (style == 0) ss << accept_count * 1.0 / (accept_count + reject_count) << "(" << accept_count << ")";
    return ss.str();
  }
  // ---- device description (this build's addition): a Gaussian with a fixed factor is drawn by the sweep kernel itself
  virtual bool device_describe(int dim, int& kind, std::vector<double>& factor, double& oneDfrac) const { return false; }
  // a set of Gaussian members that are scalar multiples of one factor: cumulative shares, scales, oneDfracs (else false)
  virtual bool device_describe_mixture(int dim, std::vector<double>& cum, std::vector<double>& scales, std::vector<double>& odfs) const { return false; }
  // differential evolution the device can draw itself (ptm_set_proposal_de): no temperature mixing, unlikely_alpha = 0; a set answers
  // for its differential-evolution member
  virtual bool device_describe_de(ptm_de_params& q) const { return false; }
  // independent draws from a distribution (draw_from_dist): the distribution, for the ladder to compare with the prior it gave the
  // engine -- the device draws from that one only (ptm_set_proposal_prior_draw); a set answers for its member; nullptr: no such draws
  virtual const sampleable_probability_function* device_draw_source() const { return nullptr; }
};

// A proposal drawn ON THE DEVICE (ptm_set_proposal_device): the engine calls draw_device once per sweep on its own stream with the
// current states of the chains that move in device memory (X_cur_dev [n_rows][dim]; rows [0, *count_dev) move, in local-chain order,
// the rest hold the other chains' states; rung_dev / walker_dev name each row's GLOBAL rung and replica; step is the ladder's step
// number); it enqueues its work on `stream` (a hipStream_t) and returns.  It writes whole proposed states to X_prop_dev and, where they
// differ from the presets 0, 0, 1, log_hastings_dev, type_dev and valid_dev.  result_device (asked for by has_result_device) sees the
// outcomes after the accept pass is queued: accepted_dev[k] in {0, 1} for k < *count_dev, the rows of the draw_device call.
// The host draw() stays required: wrapped in a proposal_distribution_set, or with PTM_DEVICE_PROPOSAL=0 in the environment, the ladder
// takes the host-proposal step and calls it once per moving chain.  With a device_likelihood the step stays on the device end to end.
// ONE clone serves every chain of a ladder on the device path (the batch holds them all).
class device_proposal : public proposal_distribution {
 public:
  virtual void draw_device(void* stream, int n_rows, int dim, const double* X_cur_dev, const int32_t* rung_dev, const int32_t* walker_dev,
                           const int32_t* count_dev, uint64_t step, double* X_prop_dev, double* log_hastings_dev, int32_t* type_dev,
                           int32_t* valid_dev) = 0;
  virtual bool has_result_device() const { return false; }
  virtual void result_device(void* stream, int n_rows, const int32_t* rung_dev, const int32_t* walker_dev, const int32_t* count_dev,
                             const int32_t* accepted_dev) {}
  state draw(state& s, chain* caller) override = 0;
  proposal_distribution* clone() const override = 0;
  std::string show() override { return "DeviceProposal()"; }
  static void device_trampoline(void* self, void* stream, int n_rows, int dim, const double* X_cur_dev, const int32_t* rung_dev,
                                const int32_t* walker_dev, const int32_t* count_dev, uint64_t step, double* X_prop_dev, double* log_hastings_dev,
                                int32_t* type_dev, int32_t* valid_dev) {
    ((device_proposal*)self)->draw_device(stream, n_rows, dim, X_cur_dev, rung_dev, walker_dev, count_dev, step, X_prop_dev, log_hastings_dev, type_dev, valid_dev);
  }
  static void device_result_trampoline(void* self, void* stream, int n_rows, const int32_t* rung_dev, const int32_t* walker_dev,
                                       const int32_t* count_dev, const int32_t* accepted_dev) {
    ((device_proposal*)self)->result_device(stream, n_rows, rung_dev, walker_dev, count_dev, accepted_dev);
  }
  // is this proposal one the ladder hands to the device as it is?  (not wrapped in a set; PTM_DEVICE_PROPOSAL=0 keeps the host path)
  static bool taken_by_device(const proposal_distribution* p) {
    const char* v = getenv("PTM_DEVICE_PROPOSAL");
    if (v && *v == '0') return false;
    return dynamic_cast<const device_proposal*>(p) != nullptr;
  }
};

namespace detail {
// a standard normal from a chain's generator (the reference: newran's Normal, newran2.cxx:164-217; replaced, not reproduced)
inline double normal_from(Random& rng) {
  const double u1 = rng.Next(), u2 = rng.Next();
  return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
}
// symmetric eigen-decomposition by cyclic Jacobi (the reference uses Eigen::SelfAdjointEigenSolver): eigenvalues ascending in
// `lambda`, eigenvectors in the columns of V (row-major n x n).  Pinned against the reference's gaussian_prop(covar) by
// tests/golden/eigen.json.gz.
inline void jacobi_eigen(std::vector<double> A, int n, std::vector<double>& lambda, std::vector<double>& V) {
  std::vector<double> Q(n * n, 0.0);
  for (int i = 0; i < n; i++) Q[i * n + i] = 1;
  for (int sweep = 0; sweep < 100; sweep++) {
    double off = 0;
    for (int p = 0; p < n; p++) for (int q = p + 1; q < n; q++) off += A[p * n + q] * A[p * n + q];
    if (off < 1e-300) break;
    for (int p = 0; p < n; p++)
      for (int q = p + 1; q < n; q++) {
        if (std::fabs(A[p * n + q]) < 1e-300) continue;
        double theta = (A[q * n + q] - A[p * n + p]) / (2 * A[p * n + q]);
        double t = (theta >= 0 ? 1 : -1) / (std::fabs(theta) + std::sqrt(theta * theta + 1));
        double c = 1 / std::sqrt(t * t + 1), sn = t * c;
        for (int k = 0; k < n; k++) { double a = A[k * n + p], b = A[k * n + q]; A[k * n + p] = c * a - sn * b; A[k * n + q] = sn * a + c * b; }
        for (int k = 0; k < n; k++) { double a = A[p * n + k], b = A[q * n + k]; A[p * n + k] = c * a - sn * b; A[q * n + k] = sn * a + c * b; }
        for (int k = 0; k < n; k++) { double a = Q[k * n + p], b = Q[k * n + q]; Q[k * n + p] = c * a - sn * b; Q[k * n + q] = sn * a + c * b; }
      }
  }
  std::vector<int> order(n);
  for (int i = 0; i < n; i++) order[i] = i;
  for (int i = 0; i < n; i++) for (int j = i + 1; j < n; j++) if (A[order[j] * n + order[j]] < A[order[i] * n + order[i]]) std::swap(order[i], order[j]);
  lambda.assign(n, 0.0); V.assign(n * n, 0.0);
  for (int j = 0; j < n; j++) {
    lambda[j] = A[order[j] * n + order[j]];
    for (int i = 0; i < n; i++) V[i * n + j] = Q[i * n + order[j]];
  }
}
}  // namespace detail

class gaussian_prop : public proposal_distribution {  // proposal_distribution.hh:145-227
  bool identity_trans;
  std::vector<double> factor;  // DIAG: sigmas; else dense D x D row-major V*diag(sqrt(lambda))
  int ndim;
  double oneDfrac;


 public:
  // factor = V * diag(sqrt(lambda)) so that offset = factor * z as in hh:207-213 (eigenvalues ascending, hh:173-176); lambda_out: the
  // eigenvalues (what ptm_eigen_factors restates on the device, and parallel_tempering_chains::adapt_gaussian_proposals' host route uses)
  static void eigen_factor(const std::vector<double>& A, int n, std::vector<double>& F, std::vector<double>* lambda_out = nullptr) {
    std::vector<double> lam, V;
    detail::jacobi_eigen(A, n, lam, V);
    F.assign(n * n, 0.0);
    for (int j = 0; j < n; j++) {
      const double sg = std::sqrt(lam[j] > 0 ? lam[j] : 0.0);
      for (int i = 0; i < n; i++) F[i * n + j] = V[i * n + j] * sg;
    }
    if (lambda_out) *lambda_out = lam;
  }

  gaussian_prop(const std::valarray<double>& sigmas, double oneDfrac = 0.0, bool scaleWithTemp = false)
      : identity_trans(true), factor(std::begin(sigmas), std::end(sigmas)), ndim(sigmas.size()), oneDfrac(oneDfrac) { check(); }
  gaussian_prop(const std::vector<double>& sigmas, double oneDfrac = 0.0, bool scaleWithTemp = false)
      : identity_trans(true), factor(sigmas), ndim(sigmas.size()), oneDfrac(oneDfrac) { check(); }
  // covariance, row-major ndim x ndim (the reference takes an Eigen::MatrixXd, hh:165)
  gaussian_prop(const std::vector<double>& covar, int ndim, double oneDfrac = 0.0, bool scaleWithTemp = false)
      : identity_trans(false), ndim(ndim), oneDfrac(oneDfrac) {
    if ((int)covar.size() != ndim * ndim) { std::cout << "gaussian_prop(constructor II): covar must be a square matrix!" << std::endl; exit(-1); }
    eigen_factor(covar, ndim, factor);
    check();
  }
  void check() const {
    if (oneDfrac < 0 || oneDfrac > 1) { std::cout << "gaussian_prop(constructor): We require 0<=oneDfrac<=1. " << std::endl; exit(1); }
  }
  gaussian_prop* clone() const override { return new gaussian_prop(*this); }
  std::string show() override {
    std::ostringstream ss;
    ss << "StepBy" << (identity_trans ? "" : "Covar") << "[dim=" << ndim << "](1Dfrac=" << oneDfrac << ")";
    return ss.str();
  }
  // gaussian_prop::draw on the host (hh:194-218) -- used when this proposal is a member of a set that cannot go to the device
  // as a whole: ndim normals first, then the optional one-dimensional move, then the transform (quirk Q4: scaleWithTemp has no
  // effect in the reference)
  state draw(state& s, chain* caller) override {
    Random& rng = *caller->getPRNG();
    std::vector<double> z(ndim);
    for (int i = 0; i < ndim; i++) z[i] = detail::normal_from(rng) * (identity_trans ? factor[i] : 1.0);
    double x = 1;
    if (oneDfrac > 0) x = rng.Next();
    if (oneDfrac > 0 && x < oneDfrac) {
      const int i = (int)(ndim * rng.Next());
      for (int j = 0; j < ndim; j++) if (j != i) z[j] = 0;
      last_type = 1;
    } else last_type = 0;
    std::vector<double> off(ndim, 0.0);
    if (identity_trans) off = z;
    else
      for (int i = 0; i < ndim; i++) { double a = 0; for (int j = 0; j < ndim; j++) a += factor[i * ndim + j] * z[j]; off[i] = a; }
    log_hastings = 0;
    return s.add(state(nullptr, off));
  }
  bool device_describe(int dim, int& kind, std::vector<double>& f, double& odf) const override {
    if (dim != ndim) { std::cout << "gaussian_prop: dimension mismatch with the chain (" << ndim << " vs " << dim << ")" << std::endl; exit(1); }
    kind = identity_trans ? PTM_PROP_DIAG : PTM_PROP_DENSE;
    f = factor;
    odf = oneDfrac;
    return true;
  }
};

// draw_from_dist (proposal_distribution.hh:119-132): an independence proposal from a sampleable distribution (the prior)
class draw_from_dist : public proposal_distribution {
  const sampleable_probability_function& dist;

 public:
  draw_from_dist(const sampleable_probability_function& dist) : dist(dist) {}
  state draw(state& s, chain* caller) override {
    state newstate = dist.drawSample(*caller->getPRNG());
    log_hastings = dist.evaluate_log(s) - dist.evaluate_log(newstate);   // likelier to draw the new state than the old one
    return newstate;
  }
  draw_from_dist* clone() const override { return new draw_from_dist(*this); }
  std::string show() override { return "DrawFrom[" + dist.show() + "]()"; }
  // the device draws from the engine's own prior: whether `dist` is that one is the ladder's to say (set_proposal)
  const sampleable_probability_function* device_draw_source() const override { return &dist; }
  // PTM_HOST_PRIOR_DRAW=1 keeps every such member on the host-proposal path (A/B timing)
  static bool kept_on_host() {
    static const bool off = [] { const char* v = getenv("PTM_HOST_PRIOR_DRAW"); return v && *v && *v != '0'; }();
    return off;
  }
};

// user_gaussian_prop (proposal_distribution.hh:236-304, .cc:259-474): a Gaussian step on a named sub-space whose covariance a
// user callback may replace before any draw.  The covariance comes as a vector: ndim variances, or the ndim (ndim+1)/2 entries of
// the upper triangle row by row; it is rescaled to the correlation matrix, diagonalised, and the step is
// diag(sigma) V (sqrt(lambda) o z) (reset_dist, .cc:340-403; negative eigenvalues are set to zero).
class user_gaussian_prop : public proposal_distribution {
 public:
  typedef bool (*check_update_prototype)(const void* parent_object, void* instance_object, const state& s, double invtemp,
                                         const std::vector<double>& randoms, std::vector<double>& covarvec);
  typedef void (*checkpoint_restart_prototype)(const void* parent_object, void* instance_object, const std::string path);
  typedef void (*accept_reject_prototype)(const void* parent_object, void* instance_object);

 private:
  std::vector<double> diagTransform;   // ndim x ndim row-major: diag(sqrt(cov_ii)) * eigenvectors of the correlation matrix
  std::vector<double> sigmas, covar_vec;
  int ndim;
  std::string label;
  check_update_prototype user_check_update;
  bool check_update_registered;
  checkpoint_restart_prototype user_checkpoint, user_restart;
  bool checkpoint_restart_registered;
  accept_reject_prototype user_accept, user_reject;
  bool accept_reject_registered;
  std::vector<int> idx_map;
  int nrand;
  bool have_dist, isverbose;

 protected:
  stateSpace domainSpace;
  void reset_dist(const std::vector<double>& covarvec) {   // .cc:340-403
    covar_vec = covarvec;
    std::vector<double> cov((size_t)ndim * ndim, 0.0);
    const int ULsize = ndim * (ndim + 1) / 2;
    if ((int)covarvec.size() == ndim) {
      for (int i = 0; i < ndim; i++) cov[i * ndim + i] = covarvec[i];
    } else if ((int)covarvec.size() == ULsize) {
      int ic = 0;
      for (int i = 0; i < ndim; i++)
        for (int j = i; j < ndim; j++) { cov[i * ndim + j] = cov[j * ndim + i] = covarvec[ic++]; }
    } else {
      std::cout << "gaussian_prop:reset_dist Covar vector has unexpeced size,ndim=" << ndim << ", UL size=" << ULsize << " but got " << covarvec.size() << " " << std::endl;
      if (have_dist) { std::cout << " Skipping update!" << std::endl; return; }
      std::cout << " Setting to identity matrix!" << std::endl;
      for (int i = 0; i < ndim; i++) cov[i * ndim + i] = 1;
    }
    std::vector<double> corr((size_t)ndim * ndim), lam, V;
    for (int i = 0; i < ndim; i++)
      for (int j = 0; j < ndim; j++) corr[i * ndim + j] = cov[i * ndim + j] / std::sqrt(cov[i * ndim + i]) / std::sqrt(cov[j * ndim + j]);
    detail::jacobi_eigen(corr, ndim, lam, V);
    diagTransform.assign((size_t)ndim * ndim, 0.0);
    sigmas.assign(ndim, 0.0);
    for (int i = 0; i < ndim; i++)
      for (int j = 0; j < ndim; j++) diagTransform[i * ndim + j] = std::sqrt(cov[i * ndim + i]) * V[i * ndim + j];
    for (int i = 0; i < ndim; i++) {
      if (lam[i] < 0) {
        std::cout << "user_gaussian_prop[" + label + "]: Warning. Negative covariance eigenvalue[" << i << "]=" << lam[i] << " set to zero." << std::endl;
        lam[i] = 0;
      }
      sigmas[i] = std::sqrt(lam[i]);
    }
    have_dist = true;
  }
  bool check_update(const state& s, chain* caller) {   // .cc:406-441
    if (!check_update_registered) return false;
    std::vector<double> randoms(nrand);
    for (auto& x : randoms) x = caller->getPRNG()->Next();
    std::vector<double> covarvec;
    const double beta = caller->invTemp();
    if (!user_check_update(user_parent_object, user_instance_object, s, beta, randoms, covarvec)) return false;
    reset_dist(covarvec);
    return true;
  }

 public:
  user_gaussian_prop(const stateSpace& sp, const std::vector<double>& covarvec = std::vector<double>(), int nrand = 0, const std::string label = "",
                     void* user_parent_object = nullptr, void* (*new_user_instance_object_function)(void* object, int id) = nullptr)
      : proposal_distribution(user_parent_object, new_user_instance_object_function), ndim(sp.size()), label(label), user_check_update(nullptr),
        check_update_registered(false), user_checkpoint(nullptr), user_restart(nullptr), checkpoint_restart_registered(false),
        user_accept(nullptr), user_reject(nullptr), accept_reject_registered(false), nrand(nrand), have_dist(false), isverbose(false), domainSpace(sp) {
    reset_dist(covarvec);
  }
  user_gaussian_prop(void* user_parent_object, check_update_prototype function, const stateSpace& sp, const std::vector<double>& covarvec = std::vector<double>(),
                     int nrand = 0, const std::string label = "", void* (*new_user_instance_object_function)(void* object, int id) = nullptr)
      : user_gaussian_prop(sp, covarvec, nrand, label, user_parent_object, new_user_instance_object_function) { register_check_update(function); }
  user_gaussian_prop* clone() const override {   // .cc:278-287: a clone asks the parent object for its own instance object
    user_gaussian_prop* c = new user_gaussian_prop(*this);
    c->id = idcount()++;
    c->set_instance();
    return c;
  }
  std::string get_label() const { return label; }
  void verbose(bool set_to = false) { isverbose = set_to; }
  void register_check_update(check_update_prototype function) { user_check_update = function; check_update_registered = true; }
  void register_checkpoint_restart(checkpoint_restart_prototype checkpointfn, checkpoint_restart_prototype restartfn) {
    user_checkpoint = checkpointfn; user_restart = restartfn; checkpoint_restart_registered = true;
  }
  void register_accept_reject(accept_reject_prototype acceptfn, accept_reject_prototype rejectfn) {
    user_accept = acceptfn; user_reject = rejectfn; accept_reject_registered = true;
  }
  state draw(state& s, chain* caller) override {   // .cc:289-338
    if (idx_map.empty()) idx_map = s.projection_indices_by_name(&domainSpace);
    std::vector<double> sparams(domainSpace.size(), 0.0);
    for (int i = 0; i < ndim; i++) if (idx_map[i] >= 0) sparams[i] = s.get_param(idx_map[i]);
    state ss = state(&domainSpace, sparams);
    last_type = check_update(ss, caller);
    Random& rng = *caller->getPRNG();
    std::vector<double> z(ndim), vec(ndim, 0.0);
    for (int i = 0; i < ndim; i++) z[i] = detail::normal_from(rng) * sigmas[i];
    for (int i = 0; i < ndim; i++) { double a = 0; for (int j = 0; j < ndim; j++) a += diagTransform[i * ndim + j] * z[j]; vec[i] = a; }
    state newstate = s.scalar_mult(0);
    for (int i = 0; i < ndim; i++) if (idx_map[i] >= 0) newstate.set_param(idx_map[i], vec[i]);
    log_hastings = 0;
    return s.add(newstate);
  }
  std::string show() override { return "StepByUserCovar[" + label + "]"; }
  void accept() override { if (accept_reject_registered) user_accept(user_parent_object, user_instance_object); accept_count++; }
  void reject() override { if (accept_reject_registered) user_reject(user_parent_object, user_instance_object); reject_count++; }
  void checkpoint(std::string path) override {   // .cc:443-458 (the covariance vector; the user's own data through its callback)
    std::ostringstream ss;
    ss << path << "user_gaussian_proposal=" << id << ".cp/";
    mkdir(ss.str().c_str(), 0777);
    std::ofstream os((ss.str() + "core_data.cp").c_str(), std::ios::binary);
    const size_t n = covar_vec.size();
    os.write((const char*)&n, sizeof n);
    os.write((const char*)covar_vec.data(), (std::streamsize)(n * 8));
    if (checkpoint_restart_registered) user_checkpoint(user_parent_object, user_instance_object, ss.str());
  }
  void restart(std::string path) override {
    std::ostringstream ss;
    ss << path << "user_gaussian_proposal=" << id << ".cp/";
    std::ifstream is((ss.str() + "core_data.cp").c_str(), std::ios::binary);
    size_t n = 0;
    is.read((char*)&n, sizeof n);
    std::vector<double> cv(n);
    is.read((char*)cv.data(), (std::streamsize)(n * 8));
    if (is) reset_dist(cv);
    if (checkpoint_restart_registered) user_restart(user_parent_object, user_instance_object, ss.str());
  }
  // without a callback the step is one fixed Gaussian: the device can draw it (factor embedded in the chain's space by
  // parameter names; rows / columns of dimensions outside the sub-space stay zero)
  bool device_describe_in(const stateSpace* full, int dim, int& kind, std::vector<double>& f, double& odf) const {
    if (check_update_registered || !full) return false;
    std::vector<int> map;
    for (int i = 0; i < ndim; i++) map.push_back(full->get_index(domainSpace.get_name(i)));
    kind = PTM_PROP_DENSE;
    f.assign((size_t)dim * dim, 0.0);
    for (int i = 0; i < ndim; i++)
      for (int j = 0; j < ndim; j++)
        if (map[i] >= 0 && map[j] >= 0) f[(size_t)map[i] * dim + map[j]] = diagTransform[i * ndim + j] * sigmas[j];
    odf = 0;
    return true;
  }
};

// proposal_distribution_set (the interface of proposal_distribution.hh:306-349): a weighted mixture of proposals.  One uniform
// of the caller's stream picks a member; its draw, log-Hastings ratio and type (reported as member + 10 x type) become the
// set's.  The weights may adapt to the members' acceptance (adapt_rate: a member that repeats its last outcome -- two accepts
// or two rejects in a row -- loses a little weight, which steers every member towards a mid-range acceptance rate; the pick
// thresholds are rebuilt every 10 x members outcomes) and may depend on the chain's temperature (Tpow, hot_shares: weight
// share + (hot_share - share)(1 - beta^Tpow)).
// On the device: members that are all gaussian_props and scalar multiples of the first one (the sampler's default Gaussian
// recipe is exactly that) -- the rung keeps ONE factor and a table of scales; anything else is drawn here, on the host.
class proposal_distribution_set : public proposal_distribution {
  struct slot {
    proposal_distribution* prop;
    double weight;       // cold share, kept normalised
    double hot_weight;   // share in the hot limit (thermal sets only)
    bool repeated;       // outcome of this member's previous proposal (accepted?)
  };
  std::vector<slot> slots;
  std::vector<double> upper;   // pick thresholds: member i is taken by a uniform below upper[i]; upper.back() == 1
  double adapt_rate, thermal_power;
  int outcomes_seen, rebuild_after, current;
  bool owner;

  // weights -> thresholds.  The weights are renormalised in place; a thermal set moves each threshold towards the hot share by
  // the chain's (1 - beta^Tpow) and then rescales so that the last threshold is exactly 1.
  void rebuild_thresholds() {
    double warm = 0;
    if (thermal_power > 0) {
      if (ch) warm = 1 - std::pow(ch->invTemp(), thermal_power);
      else std::cout << "proposal_distribution_set: temperature-dependent shares need the chain (set_chain) -- using the cold shares." << std::endl;
    }
    double total = 0;
    for (size_t i = 0; i < slots.size(); i++) total += slots[i].weight;
    double edge = 0;
    for (size_t i = 0; i < slots.size(); i++) {
      slot& m = slots[i];
      m.weight /= total;
      edge = edge + m.weight;
      if (thermal_power > 0) edge += (m.hot_weight - m.weight) * warm;
      upper[i] = edge;
    }
    const double top = upper.back();
    for (size_t i = 0; i < upper.size(); i++) upper[i] /= top;
  }
  // bookkeeping shared by accept() and reject()
  void outcome(bool accepted) {
    slot& m = slots[current];
    if (adapt_rate != 0) {
      if (m.repeated == accepted) m.weight *= 1 - adapt_rate * 0.25;
      m.repeated = accepted;
      if (++outcomes_seen >= rebuild_after) rebuild_thresholds();
    }
    if (accepted) m.prop->accept(); else m.prop->reject();
  }
  std::vector<double> weights(bool hot) const {
    std::vector<double> w(slots.size());
    for (size_t i = 0; i < slots.size(); i++) w[i] = hot ? slots[i].hot_weight : slots[i].weight;
    return w;
  }

 public:
  // takes the pointers (take_pointers = true, the reference's default: the set deletes its members); clone() deep-copies
  proposal_distribution_set(const std::vector<proposal_distribution*>& props, const std::vector<double>& shares_, double adapt_rate = 0, double Tpow = 0,
                            std::vector<double> hot_shares_ = std::vector<double>(), bool take_pointers = true)
      : adapt_rate(adapt_rate), thermal_power(Tpow), outcomes_seen(0), rebuild_after(10 * (int)props.size()), current(0), owner(take_pointers) {
    if (props.empty() || props.size() != shares_.size()) { std::cout << "proposal_distribution_set: " << props.size() << " proposals but " << shares_.size() << " shares." << std::endl; exit(1); }
    bool hot_ok = false;
    double hot_total = 0;
    if (Tpow > 0) {
      for (size_t i = 0; i < hot_shares_.size(); i++) hot_total += hot_shares_[i];
      hot_ok = hot_shares_.size() == props.size() && hot_total > 0;
      if (!hot_ok) std::cout << "proposal_distribution_set: Tpow > 0 needs one hot share per member with a positive sum -- using the cold shares." << std::endl;
    }
    for (size_t i = 0; i < props.size(); i++) {
      slot m;
      m.prop = props[i]; m.weight = shares_[i]; m.repeated = true;
      m.hot_weight = Tpow > 0 ? (hot_ok ? hot_shares_[i] / hot_total : shares_[i]) : 0.0;
      slots.push_back(m);
    }
    upper.assign(slots.size(), 0.0);
    rebuild_thresholds();
    last_type = 0;
  }
  ~proposal_distribution_set() { if (owner) for (size_t i = 0; i < slots.size(); i++) delete slots[i].prop; }
  proposal_distribution_set(const proposal_distribution_set&) = delete;
  proposal_distribution_set* clone() const override {
    std::vector<proposal_distribution*> copies;
    for (size_t i = 0; i < slots.size(); i++) copies.push_back(slots[i].prop->clone());
    proposal_distribution_set* c = new proposal_distribution_set(copies, weights(false), adapt_rate, thermal_power, weights(true), true);
    for (size_t i = 0; i < slots.size(); i++) c->slots[i].repeated = slots[i].repeated;
    c->outcomes_seen = outcomes_seen;
    return c;
  }
  void set_chain(chain* c) override {
    ch = c;
    for (size_t i = 0; i < slots.size(); i++) slots[i].prop->set_chain(c);
    rebuild_thresholds();   // (a thermal set now knows its temperature)
  }
  bool support_mixing() override {
    for (size_t i = 0; i < slots.size(); i++) if (slots[i].prop->support_mixing()) return true;
    return false;
  }
  // The pick: a set of one member draws no uniform (so that it IS its member, random stream included); otherwise the first
  // member that is ready and whose threshold lies above the uniform.  If the uniform falls to members that are not ready
  // (differential evolution before its history is long enough) another uniform is drawn -- a hundred times at most.
  state draw(state& s, chain* caller) override {
    Random& rng = *caller->getPRNG();
    for (int attempt = 0; attempt <= 100; attempt++) {
      const double u = slots.size() > 1 ? rng.Next() : 0.0;
      for (size_t i = 0; i < slots.size(); i++) {
        proposal_distribution* p = slots[i].prop;
        if (!(u < upper[i]) || !p->is_ready()) continue;
        state proposed = p->draw(s, caller);
        log_hastings = p->log_hastings_ratio();
        last_type = (int)i + 10 * p->type();
        current = (int)i;
        return proposed;
      }
    }
    std::cout << "proposal_distribution_set::draw: no member was ready to draw in 100 attempts." << std::endl;
    exit(1);
  }
  void accept() override { proposal_distribution::accept(); outcome(true); }
  void reject() override { proposal_distribution::reject(); outcome(false); }
  void checkpoint(std::string path) override { for (size_t i = 0; i < slots.size(); i++) slots[i].prop->checkpoint(path); }
  void restart(std::string path) override { for (size_t i = 0; i < slots.size(); i++) slots[i].prop->restart(path); }
  std::string show() override {
    std::ostringstream ss;
    ss << "ChooseFrom(";
    for (size_t i = 0; i < slots.size(); i++) ss << "  " << (upper[i] - (i ? upper[i - 1] : 0.0)) * 100. << "% : " << slots[i].prop->show() << "\n";
    ss << ")\n";
    return ss.str();
  }
  // style 0: acceptance of the set and of every member; style 1: the current pick probabilities
  std::string report(int style = 0) override {
    std::ostringstream ss;
    if (style == 0) {
      ss << proposal_distribution::report(0) << ":[";
      for (size_t i = 0; i < slots.size(); i++) ss << (i ? "," : "") << slots[i].prop->report(0);
      ss << "]";
    } else if (style == 1) {
      ss << "shares=[";
      for (size_t i = 0; i < slots.size(); i++) {
        ss << (i ? "," : "") << upper[i] - (i ? upper[i - 1] : 0.0);
        const std::string inner = slots[i].prop->report(1);
        if (!inner.empty()) ss << ":" << inner;
      }
      ss << "]";
    }
    return ss.str();
  }
  std::vector<proposal_distribution*> members() const {
    std::vector<proposal_distribution*> v;
    for (size_t i = 0; i < slots.size(); i++) v.push_back(slots[i].prop);
    return v;
  }
  // the member that is a differential evolution the device can draw (at most one, and not the last: a member that is not ready is
  // passed over for the NEXT one, proposal_distribution.cc:111), or -1
  int device_de_member() const {
    int at = -1;
    for (size_t i = 0; i < slots.size(); i++) {
      ptm_de_params q;
      if (!slots[i].prop->device_describe_de(q)) continue;
      if (at >= 0 || i + 1 == slots.size()) return -2;   // two of them, or nothing behind it: the host's business
      at = (int)i;
    }
    return at;
  }
  // the member that draws from a distribution (draw_from_dist; -1: none, -2: more than one or PTM_HOST_PRIOR_DRAW).  The device draws
  // it if the distribution is the engine's prior (ptm_set_proposal_prior_draw), which the ladder checks (device_draw_source)
  int device_prior_member() const {
    int at = -1;
    for (size_t i = 0; i < slots.size(); i++) {
      if (dynamic_cast<const proposal_distribution_set*>(slots[i].prop) || !slots[i].prop->device_draw_source()) continue;
      if (at >= 0 || draw_from_dist::kept_on_host()) return -2;
      at = (int)i;
    }
    return at;
  }
  const sampleable_probability_function* device_draw_source() const override {
    const int pm = device_prior_member();
    return pm >= 0 ? slots[pm].prop->device_draw_source() : nullptr;
  }
  // a draw_from_dist anywhere the device cannot take it: inside a nested set, two of them, or kept on the host by the environment
  bool prior_draws_need_host() const {
    if (device_prior_member() == -2) return true;
    for (size_t i = 0; i < slots.size(); i++) {
      const proposal_distribution_set* in = dynamic_cast<const proposal_distribution_set*>(slots[i].prop);
      if (in && (in->device_prior_member() != -1 || in->prior_draws_need_host())) return true;
    }
    return false;
  }
  int first_gaussian_member() const {
    const int de = device_de_member(), pm = device_prior_member();
    for (size_t i = 0; i < slots.size(); i++) if ((int)i != de && (int)i != pm) return (int)i;
    return -1;
  }
  // temperature-dependent shares (Tpow > 0): the device takes them from a set whose TOP shares do not adapt -- every rung's clone hands
  // over the thresholds it built at set_chain, and nothing rebuilds them; an adapting thermal set stays on the host
  bool thermal_on_host() const { return thermal_power > 0 && adapt_rate != 0; }
  bool thermal() const { return thermal_power > 0; }
  bool device_describe_de(ptm_de_params& q) const override {
    const int de = device_de_member();
    return de >= 0 && (adapt_rate == 0 || adaptive()) && !thermal_on_host() && slots[de].prop->device_describe_de(q);
  }
  bool device_describe(int dim, int& kind, std::vector<double>& f, double& odf) const override {
    if (thermal_on_host() || prior_draws_need_host()) return false;
    if (adaptive()) {                      // shares that move: the device's adaptive set (device_describe_adaptive)
      ptm_adaptive_set a;
      std::vector<double> sc, od;
      odf = 0;
      return device_describe_adaptive(dim, kind, f, a, sc, od);
    }
    if (adapt_rate != 0) return false;
    const int g0 = first_gaussian_member();
    if (device_de_member() == -2 || g0 < 0 || !slots[g0].prop->device_describe(dim, kind, f, odf)) return false;
    std::vector<double> cum, sc, od;
    if (!device_describe_mixture(dim, cum, sc, od)) return false;
    odf = 0;   // the members' oneDfracs live in the mixture table
    return true;
  }
  // Gaussian members that are scalar multiples of one factor, and at most one differential evolution (scale -1: ptm_set_proposal_de)
  bool device_describe_mixture(int dim, std::vector<double>& cum, std::vector<double>& scales, std::vector<double>& odfs) const override {
    if (adapt_rate != 0 || adaptive() || prior_draws_need_host()) return false;
    const int de = device_de_member(), g0 = first_gaussian_member(), pm = device_prior_member();
    if (de == -2 || g0 < 0) return false;
    int kind0; double odf0; std::vector<double> f0;
    if (!slots[g0].prop->device_describe(dim, kind0, f0, odf0)) return false;
    cum.clear(); scales.clear(); odfs.clear();
    for (size_t i = 0; i < slots.size(); i++) {
      cum.push_back(i + 1 == slots.size() ? 1.0 : upper[i]);
      if ((int)i == de) { scales.push_back(-1.0); odfs.push_back(0.0); continue; }
      if ((int)i == pm) { scales.push_back(1.0); odfs.push_back(0.0); continue; }   // (neither is read: ptm_set_proposal_prior_draw)
      int kind; double odf; std::vector<double> f;
      if (!slots[i].prop->device_describe(dim, kind, f, odf) || kind != kind0 || f.size() != f0.size()) return false;
      double sc = 0;
      for (size_t k = 0; k < f.size(); k++) if (f0[k] != 0) { sc = f[k] / f0[k]; break; }
      for (size_t k = 0; k < f.size(); k++)
        if (std::fabs(f[k] - sc * f0[k]) > 1e-12 * (std::fabs(f[k]) + std::fabs(sc * f0[k])) + 1e-300) return false;   // not a multiple
      scales.push_back(sc);
      odfs.push_back(odf);
    }
    return true;
  }
  // ---- adaptive sets on the device (ptm_set_proposal_adaptive) ----
  // the member that is itself a proposal_distribution_set (-1: none, -2: more than one)
  int nested_member() const {
    int at = -1;
    for (size_t i = 0; i < slots.size(); i++)
      if (dynamic_cast<const proposal_distribution_set*>(slots[i].prop)) {
        if (at >= 0) return -2;
        at = (int)i;
      }
    return at;
  }
  // do this set's shares, or those of a nested set, adapt?
  bool adaptive() const {
    if (adapt_rate != 0) return true;
    const int n = nested_member();
    return n >= 0 && ((const proposal_distribution_set*)slots[n].prop)->adapt_rate != 0;
  }
  // The adaptive set the device draws: Tpow = 0 unless the top shares stay fixed, up to eight top members -- at most one differential evolution that is not the last
  // (scale -1), at most one nested adaptive set of Gaussians, and single Gaussians --, every Gaussian a scalar multiple of one factor
  // (kind, f: the first Gaussian's).  Leaves: the top members, then the nested set's; the nested member's own entry is 1.
  bool device_describe_adaptive(int dim, int& kind, std::vector<double>& f, ptm_adaptive_set& a, std::vector<double>& scales,
                                std::vector<double>& odfs) const {
    if (thermal_on_host() || prior_draws_need_host() || !adaptive() || slots.size() > 8) return false;
    const int nest = nested_member(), de = device_de_member(), pm = device_prior_member();
    if (nest == -2 || de == -2 || (nest >= 0 && nest == de)) return false;
    const proposal_distribution_set* in = nest >= 0 ? (const proposal_distribution_set*)slots[nest].prop : nullptr;
    if (in && (in->thermal_power > 0 || in->slots.size() > 8 || in->nested_member() != -1 || in->device_de_member() != -1)) return false;
    std::vector<const proposal_distribution*> gauss;   // every Gaussian leaf, in leaf order
    for (size_t i = 0; i < slots.size(); i++)
      if ((int)i != de && (int)i != nest && (int)i != pm) gauss.push_back(slots[i].prop);
    if (in)
      for (size_t j = 0; j < in->slots.size(); j++) gauss.push_back(in->slots[j].prop);
    if (gauss.empty()) return false;
    double odf0;
    if (!gauss[0]->device_describe(dim, kind, f, odf0)) return false;
    auto scale_of = [&](const proposal_distribution* p, double& sc, double& odf) {
      int k;
      std::vector<double> g;
      if (dynamic_cast<const proposal_distribution_set*>(p) || !p->device_describe(dim, k, g, odf) || k != kind || g.size() != f.size()) return false;
      sc = 0;
      for (size_t i = 0; i < g.size(); i++) if (f[i] != 0) { sc = g[i] / f[i]; break; }
      for (size_t i = 0; i < g.size(); i++)
        if (std::fabs(g[i] - sc * f[i]) > 1e-12 * (std::fabs(g[i]) + std::fabs(sc * f[i])) + 1e-300) return false;   // not a multiple
      return true;
    };
    scales.clear(); odfs.clear();
    for (size_t i = 0; i < slots.size(); i++) {
      double sc = 1.0, odf = 0.0;
      if ((int)i == de) sc = -1.0;
      else if ((int)i != nest && (int)i != pm && !scale_of(slots[i].prop, sc, odf)) return false;
      scales.push_back(sc); odfs.push_back(odf);
    }
    if (in)
      for (size_t j = 0; j < in->slots.size(); j++) {
        double sc, odf;
        if (!scale_of(in->slots[j].prop, sc, odf)) return false;
        scales.push_back(sc); odfs.push_back(odf);
      }
    a.K = (int)slots.size(); a.nested = nest; a.K_inner = in ? (int)in->slots.size() : 0;
    a.rate = adapt_rate; a.rate_inner = in ? in->adapt_rate : 0.0;
    return true;
  }
  // this set's adaptive state and its nested set's, in the rows of ptm_set_proposal_adaptive / ptm_get_proposal_adapt_state:
  // weights, thresholds [K + K_inner]; bits of the members whose last outcome was an accept, outcome counts [2] (top, nested)
  void adapt_state(std::vector<double>& w, std::vector<double>& th, std::vector<int>& bits, std::vector<int>& cnt) const {
    w.clear(); th.clear(); bits.assign(2, 0); cnt.assign(2, 0);
    const int nest = nested_member();
    const proposal_distribution_set* in = nest >= 0 ? (const proposal_distribution_set*)slots[nest].prop : nullptr;
    for (int b = 0; b < (in ? 2 : 1); b++) {
      const proposal_distribution_set* s = b ? in : this;
      for (size_t i = 0; i < s->slots.size(); i++) {
        w.push_back(s->slots[i].weight); th.push_back(s->upper[i]);
        if (s->slots[i].repeated) bits[b] |= 1 << i;
      }
      cnt[b] = s->outcomes_seen;
    }
  }
  // ... and back (the device's state, for the report)
  void set_adapt_state(const double* w, const double* th, const int32_t* bits, const int32_t* cnt) {
    const int nest = nested_member();
    proposal_distribution_set* in = nest >= 0 ? (proposal_distribution_set*)slots[nest].prop : nullptr;
    size_t k = 0;
    for (int b = 0; b < (in ? 2 : 1); b++) {
      proposal_distribution_set* s = b ? in : this;
      for (size_t i = 0; i < s->slots.size(); i++, k++) {
        s->slots[i].weight = w[k]; s->upper[i] = th[k];
        s->slots[i].repeated = ((bits[b] >> i) & 1) != 0;
      }
      s->outcomes_seen = cnt[b];
    }
  }
};

// differential_evolution (the interface of proposal_distribution.hh:351-414): DE-MC with sampling from the past, ter Braak &
// Vrugt, Stat. Comput. 18 (2008) 435 -- the jump is a multiple of the difference of two states drawn from the saved history.
//   parallel-direction move (eq. 2):  x* = x + gamma (z1 - z2),  gamma = 1.68 / sqrt(d) / reduce_gamma, or 1 with probability
//                                     gamma_one_frac (unit jumps hop between modes); symmetric, log-Hastings 0, type 0
//   snooker move (eq. 3-4):           z drawn from the history (until z != x), x* = x + gamma ((z1 - z2) . e) e / |e|^2 with
//                                     e = x - z, gamma uniform on (1.2, 2.2) / reduce_gamma; log-Hastings
//                                     (d - 1)/2 (ln |x* - z|^2 - ln |x - z|^2), type 1
// How the reference's implementation behaves (proposal_distribution.cc:476-801), and this one with it -- pinned draw by draw
// against the reference by tests/golden/trace13.json.gz:
//   * rows are taken uniformly from the RAW history [start, size): start > 0 only once (size - 100 d)(1 - ignore_frac) > 10 d,
//     then start = (size - 100 d) ignore_frac; the proposal is ready when the history holds 10 d rows;
//   * unlikely_alpha > 0: a row whose log-posterior lies below (MAP - d) is kept with probability exp(alpha (lpost - MAP + d)),
//     alpha shrinking by 0.9 per refusal.  The MAP and the log-posteriors are those of the proposal's OWN chain (set_chain),
//     also when the row index was drawn for the length of another rung's history;
//   * support_mixing: each history state comes from a rung of the ladder picked with weight exp(min(0, -(L0 - a Lmed) / mix)),
//     a = beta_caller - beta_rung, L0 = ln mean exp(a l) over ten rows (log-likelihoods read from the CALLER's history at
//     indices drawn for the rung's length, non-finite ones redrawn), Lmed the median (6th of 10, sorted) of ten of the rung's
//     own log-likelihoods;
//   * the small Gaussian jump of eq. 2 (b_small) is drawn by the reference and then dropped (its sum is never assigned), so no
//     proposal depends on it: it is not drawn here.
// Needs the chain history -- on this build the ladder keeps a host mirror of what MH_chain::add_state saves when a host-side
// proposal is in use (parallel_tempering_chains::sync_history).
class differential_evolution : public proposal_distribution {
  double p_snooker, p_unit_gamma, jump_noise, skip_early, discount, gamma_divisor, mix_strength;
  bool mixing, bound_to_chain;
  int d;

  int rows_to_start() const { return 10 * d; }
  int rows_before_skipping() const { return 100 * d; }
  void must_be_ready() {
    if (is_ready()) return;
    if (bound_to_chain) std::cout << "differential_evolution: the history holds " << ch->size() << " rows, " << rows_to_start() << " are needed" << std::endl;
    else std::cout << "differential_evolution: no chain was set" << std::endl;
    std::cout << "differential_evolution: drawing before is_ready() -- check is_ready() first." << std::endl;
    exit(1);
  }
  // a raw row index of `source`'s history, by the uniforms of `who`
  int pick_row(chain* who, chain* source) {
    must_be_ready();
    Random& u = *who->getPRNG();
    const int rows = source->size();
    const int spare = rows - rows_before_skipping();
    const int first = spare * (1 - skip_early) > rows_to_start() ? (int)(spare * skip_early) : 0;
    const double floor_lpost = ch->getMAPlpost() - ch->getDim();
    for (double strictness = discount;; strictness *= 0.9) {
      const int row = (int)(first + (rows - first) * u.Next());
      if (!(strictness > 0)) return row;
      const double lpost = ch->getLogPost(row, true);
      if (!(floor_lpost > lpost)) return row;
      if (u.Next() < std::exp(strictness * (lpost - floor_lpost))) return row;
    }
  }
  // weight of rung `rung` as a source of history for a caller at inverse temperature beta_caller
  double rung_weight(chain* who, chain* rung, double beta_caller, bool& same_temperature) {
    const int nprobe = 10;
    double probe[nprobe], lo = 1e100, hi = -1e100;
    for (int got = 0; got < nprobe;) {
      const double l = who->getLogLike(pick_row(who, rung), true);
      if (!std::isfinite(l)) continue;
      if (l > hi) hi = l;
      if (l < lo) lo = l;
      probe[got++] = l;
    }
    const double a = -(rung->invTemp() - beta_caller);
    same_temperature = a == 0;
    const double pivot = a < 0 ? lo : hi;   // keeps every exponent below <= 0
    double acc = 0;
    for (int i = 0; i < nprobe; i++) acc += std::exp((probe[i] - pivot) * a);
    const double log_mean = std::log(acc / nprobe) + pivot * a;
    std::vector<double> own(nprobe);
    for (int i = 0; i < nprobe; i++) own[i] = rung->getLogLike(pick_row(who, rung), true);
    std::sort(own.begin(), own.end());
    double lw = -(log_mean - own[nprobe / 2] * a);
    lw /= mix_strength;
    return std::exp(lw > 0 ? 0.0 : lw);
  }
  // one state of the history, as a parameter vector
  std::vector<double> pick_state(chain* who) {
    must_be_ready();
    const int nrungs = ch->multiplicity();
    if (nrungs == 1 || !mixing) return ch->getState(pick_row(who, ch), true).get_params_vector();
    std::vector<double> reach(nrungs + 1, 0.0);
    const double beta = who->invTemp();
    int own_rung = 0;
    for (int r = 0; r < nrungs; r++) {
      bool same = false;
      reach[r + 1] = reach[r] + rung_weight(who, ch->subchain(r), beta, same);
      if (same) own_rung = r;
    }
    const double mark = who->getPRNG()->Next() * reach[nrungs];
    int from = own_rung;
    for (int r = 0; r < nrungs; r++) if (mark <= reach[r + 1]) { from = r; break; }
    chain* rung = ch->subchain(from);
    return rung->getState(pick_row(who, rung), true).get_params_vector();
  }
  static double dot(const std::vector<double>& a, const std::vector<double>& b) {
    double t = 0;
    for (size_t i = 0; i < a.size(); i++) t += a[i] * b[i];
    return t;
  }
  // v + c w, elementwise (the product rounded before the sum, as state::scalar_mult followed by state::add does it)
  static std::vector<double> plus_scaled(const std::vector<double>& v, const std::vector<double>& w, double c) {
    std::vector<double> r(v.size());
    for (size_t i = 0; i < v.size(); i++) { const double t = w[i] * c; r[i] = v[i] + t; }
    return r;
  }
  state parallel_move(state& s, chain* who) {
    Random& u = *who->getPRNG();
    const double gamma = u.Next() < p_unit_gamma ? 1.0 : 1.68 / std::sqrt((double)d) / gamma_divisor;
    const std::vector<double> z1 = pick_state(who), z2 = pick_state(who);
    std::vector<double> x = plus_scaled(s.get_params_vector(), z1, gamma);
    x = plus_scaled(x, z2, -gamma);
    log_hastings = 0;
    last_type = 0;
    return s.moved_to(x);
  }
  state snooker_move(state& s, chain* who) {
    const double gamma = (1.2 + who->getPRNG()->Next()) / gamma_divisor;
    const std::vector<double> x = s.get_params_vector();
    std::vector<double> z, axis;
    double axis2 = 0;
    for (int tries = 0; axis2 == 0; tries++) {   // the history repeats states: the projection needs a z that is not x itself
      if (tries > 1000) { std::cout << "differential_evolution: a thousand history states in a row equal the current state; giving up." << std::endl; exit(1); }
      z = pick_state(who);
      axis = plus_scaled(x, z, -1.0);
      axis2 = dot(axis, axis);
    }
    const std::vector<double> z1 = pick_state(who), z2 = pick_state(who);
    std::vector<double> diff(x.size());
    for (size_t i = 0; i < diff.size(); i++) { const double a = z1[i] * gamma, b = z2[i] * (-gamma); diff[i] = a + b; }
    const std::vector<double> y = plus_scaled(x, axis, dot(diff, axis) / axis2);
    const std::vector<double> from_z = plus_scaled(y, z, -1.0);
    log_hastings = (std::log(dot(from_z, from_z)) - std::log(axis2)) * (d - 1) / 2.0;
    last_type = 1;
    return s.moved_to(y);
  }

 public:
  differential_evolution(double snooker = 0.0, double gamma_one_frac = 0.1, double b_small = 0.0001, double ignore_frac = 0.3, double unlikely_alpha = 0)
      : p_snooker(snooker), p_unit_gamma(gamma_one_frac), jump_noise(b_small), skip_early(ignore_frac), discount(unlikely_alpha), gamma_divisor(1),
        mix_strength(1), mixing(false), bound_to_chain(false), d(0) {}
  void reduce_gamma(double factor) { gamma_divisor = factor; }
  void mix_temperatures_more(double factor) { mix_strength = factor; }
  void set_chain(chain* c) override { ch = c; bound_to_chain = true; d = c->getDim(); }
  bool is_ready() override { return bound_to_chain && ch->size() >= rows_to_start(); }
  state draw(state& s, chain* caller) override { return p_snooker > caller->getPRNG()->Next() ? snooker_move(s, caller) : parallel_move(s, caller); }
  differential_evolution* clone() const override { return new differential_evolution(*this); }
  std::string show() override {
    std::ostringstream ss;
    ss << "DifferentialEvolution(snooker=" << p_snooker << ", gamma_one_frac=" << p_unit_gamma << ", b_small=" << jump_noise << ", ignore_frac=" << skip_early << ")\n";
    return ss.str();
  }
  bool support_mixing(bool do_it) { mixing = do_it; return do_it; }
  bool support_mixing() override { return mixing; }
  // what the engine draws on the device from its own history (ptm_set_proposal_de): everything but temperature mixing and
  // unlikely_alpha, which stay with this class on the host
  bool device_describe_de(ptm_de_params& q) const override {
    static const bool off = [] { const char* v = getenv("PTM_HOST_DE"); return v && *v && *v != '0'; }();   // (A/B timing: keep the host path)
    if (off || mixing || discount != 0) return false;
    q.snooker = p_snooker; q.gamma_one_frac = p_unit_gamma; q.reduce_gamma = gamma_divisor; q.ignore_frac = skip_early;
    return true;
  }
};

// ---- effective sample size of a saved series ---------------------------------------------------------------------------------
// The estimator behind chain::report_effective_samples (chain.cc:126-643) and the sampler's --chain_ess_stop, restated on a
// plain series so that it can be checked on its own (tests/golden/ess.json.gz holds the reference's answers for fixed AR(1)
// series).  In the manner of Geyer (1992), "Practical Markov chain Monte Carlo", sec. 3:
//   * the last part of the series is cut into windows of `width` steps that end at the newest step, each sampled every
//     `every` steps; `burn` more windows in front of them only feed the lagged samples;
//   * per window and lag L (0, then every, 2 every, ... spaced by factors of 1.1 up to burn windows): the mean m of the
//     samples and their L-lagged partners taken together, and the lagged covariance about m;
//   * for the newest n windows together: rho(L) = sum count (cov_L + (M - m_L)^2) / sum count (cov_0 + (M - m_0)^2), M the mean
//     of the window means; autocorrelation length 1 + 2 sum (L_k - L_(k-1)) rho(L_k), stopped -- and the last term taken back --
//     at the second negative rho in a row (the initially positive sequence);
//   * ess(n) = n width / length (a length below the sampling stride is not believed: 3 strides are assumed instead), the
//     minimum over the features; the answer is the best n: early windows lengthen the correlation more than they add samples.
// report() chooses width / stride like the reference: windows doubled until at most 20 + 2 of them cover the series, or, given
// a limit on the ess worth resolving, a search from coarse to fine strides.
// The pass with fixed windows can be handed to a backend (use_backend): the engine's kernels run it on the device's own history
// ring, in this very order of operations -- same bits (ptm_ess_windowed); report() stays the one implementation of the search.
class ess_estimator {
 public:
  // features of the state saved for nominal step `step` (false: none, the sample is skipped)
  typedef std::function<bool(int step, std::vector<double>& features)> reader;
  // windowed(width, every, burn) computed elsewhere
  typedef std::function<void(int width, int every, int burn, double& ess, int& nwin)> window_backend;

 private:
  int steps, nfeat;
  reader read;
  window_backend backend;
  bool sample(int step, std::vector<double>& v) const { return step >= 0 && step < steps && read(step, v) && (int)v.size() >= nfeat; }

  struct cell { double mean, cov; int count; };

 public:
  ess_estimator(int steps, int nfeat, reader read) : steps(steps), nfeat(nfeat), read(read) {}
  void use_backend(window_backend b) { backend = b; }

  // one pass with fixed windows: ess and the number of windows that gave it
  void windowed(int width, int every, int burn, double& ess_out, int& nwin_out) const {
    ess_out = 0; nwin_out = 0;
    if (backend) { backend(width, every, burn, ess_out, nwin_out); return; }
    if (width < 2) width = 2;
    if (every < 1) every = 1;
    if (burn < 1) burn = 1;
    const int per_window = width / every, span = per_window * every;   // samples per window, steps they cover
    if (per_window < 1) return;
    int nwin = steps / span - burn;
    if (nwin < 1) return;
    const int origin = steps - nwin * span;
    std::vector<int> lags(1, 0);
    {
      double grow = 1;
      for (int k = 1; k < burn * per_window;) {
        lags.push_back(every * k);
        const int was = k;
        while (k == was) { grow *= 1.1; k = (int)grow; }
      }
    }
    const int nlag = (int)lags.size();
    // table[f][w][l]
    std::vector<std::vector<std::vector<cell> > > table(nfeat, std::vector<std::vector<cell> >(nwin, std::vector<cell>(nlag)));
    std::vector<double> now, then;
    std::vector<std::vector<double> > base(per_window);
    std::vector<char> have(per_window);
    for (int w = 0; w < nwin; w++) {
      const int w0 = origin + w * span;
      for (int i = 0; i < per_window; i++) have[i] = sample(w0 + i * every, base[i]) ? 1 : 0;
      for (int l = 0; l < nlag; l++) {
        std::vector<double> s1(nfeat, 0.0), s2(nfeat, 0.0);
        int n = 0;
        for (int i = 0; i < per_window; i++) {
          if (!have[i]) continue;
          if (l == 0) {
            for (int f = 0; f < nfeat; f++) { s1[f] += base[i][f]; s2[f] += base[i][f] * base[i][f]; }
          } else {
            if (!sample(w0 + i * every - lags[l], then)) continue;
            for (int f = 0; f < nfeat; f++) { s1[f] += then[f] + base[i][f]; s2[f] += then[f] * base[i][f]; }
          }
          n++;
        }
        for (int f = 0; f < nfeat; f++) {
          cell& c = table[f][w][l];
          c.count = n;
          c.mean = l == 0 ? s1[f] / n : s1[f] / n / 2;
          c.cov = s2[f] / n - c.mean * c.mean;
        }
      }
    }
    for (int n = 1; n <= nwin; n++) {
      double worst = 1e100;
      for (int f = 0; f < nfeat; f++) {
        double msum = 0;
        for (int w = nwin - n; w < nwin; w++) msum += table[f][w][0].mean;
        const double M = msum / n;
        double length = 1.0, last_term = 0, previous = 1;
        int last_lag = 0;
        for (int l = 1; l < nlag; l++) {
          double top = 0, bottom = 0;
          for (int w = nwin - n; w < nwin; w++) {
            const cell &c = table[f][w][l], &c0 = table[f][w][0];
            const double dm = M - c.mean, dm0 = M - c0.mean;
            const double cv = c.cov + dm * dm, var = c0.cov + dm0 * dm0;
            top += cv * c.count;
            bottom += var * c.count;
          }
          const double rho = top / bottom;
          if (previous < 0 && rho < 0) { length -= last_term; break; }
          previous = rho;
          last_term = 2.0 * (lags[l] - last_lag) * rho;
          length += last_term;
          last_lag = lags[l];
        }
        double e = n * width / length;
        if (length < every) e = n * width / 3.0 / every;
        if (e < worst) worst = e;
      }
      if (worst > ess_out) { ess_out = worst; nwin_out = n; }
    }
  }

  // (ess, useful length of the series in steps).  width: first guess of the window; every: sampling stride (< 0: the stride the
  // series was saved with, from its rows and its initial rows); esslimit < 0: no limit
  std::pair<double, int> report(int width, int every, double esslimit, int rows = 0, int initial_rows = 0) const {
    const int min_burn = 2, min_per_window = 1000, max_windows = 20;
    while (width < steps * 0.05) width *= 2;
    if (every < 0) every = rows > initial_rows ? (int)(0.5 + ((double)steps - initial_rows) / (rows - initial_rows)) : 1;
    if (every < 1) every = 1;
    double ess = 0, best_width = 0;
    int nwin = 0;
    if (esslimit < 0) {
      if (width < 0) width = every * min_per_window;
      while (width * (max_windows + min_burn) < steps) width *= 2;
      windowed(width, every, min_burn, ess, nwin);
      best_width = width;
    } else {
      // An ess above the limit need not be resolved, so a long series is first looked at with a coarse stride (cheap) and the
      // stride refined only while the limit, not the series' length, decides the window: a window should hold ~1000 samples,
      // the newest <= 20 windows are used, and limit x 3 strides is the longest stretch whose ess could still matter.
      const double length = steps, reach = esslimit * 3.0;
      for (bool last_round = false; !last_round; every *= 2) {
        int windows = (int)(length / (min_per_window * every));
        if (windows > max_windows) windows = max_windows;
        if (windows < 1) break;
        width = (int)(length / windows);
        if (width * (windows - 1) > reach * every) {
          windows = (int)(reach / min_per_window + 1);
          if (windows > max_windows) windows = max_windows;
          if (windows > 1) width = (int)((reach * every) / (windows - 1));
          else { windows = 1; width = min_per_window * every; }
        } else last_round = true;
        if ((length - length / (max_windows + min_burn)) * 0.5 < windows * width) {
          double e; int n;
          windowed(width, every, (int)(length / width - windows), e, n);
          if (e > ess) { ess = e; nwin = n; best_width = width; }
        }
      }
    }
    return std::make_pair(ess, (int)best_width * nwin);
  }
};

// ---- log-evidence by thermodynamic integration over the ladder (chain.cc:1577-1676, 1984-2012) ----------------------------------
// evidence_estimator: parallel_tempering_chains::log_evidence_ratio and the total of the statistics block, on plain arrays.
//   * the window of chain b is MH_chain::get_state_idx (chain.cc:1041-1049) of Nhist - ilen and of Nhist -- an index outside
//     [0, Nhist) becomes Nhist - 1 --: saved rows [1 + (Nhist - ilen) / add_every_N, 1 + (Nhist - 1) / add_every_N) in the ring's
//     numbering (row 0 the start state).  So the newest saved row is left out and a chain with Nhist < ilen has no row: 0 / 0.
//   * ratio(a, b) = sum of llike_b[row] * (beta_a - beta_b) in row order / count (chain.cc:1998-2007): multiply, then add;
//   * up[i] = ratio(i, i+1), down[i] = -ratio(i+1, i), evidence += (up[i] + down[i]) / 2.0 in that order, then the term of the last
//     pair / (beta[Nt-2] / beta[Nt-1] - 1) for what lies below the hottest rung (chain.cc:1586-1597).
// The engine's kernels run the same operations in the same order on the device's own ring (ptm_log_evidence): same bits.
class evidence_estimator {
 public:
  // llike of saved row `row` (the ring's numbering) of rung `rung`; false: the row is not there any more
  typedef std::function<bool(int rung, long long row, double& llike)> reader;
  struct result {
    double evidence;
    std::vector<double> up, down;   // [Nt - 1]
    std::vector<int> count;         // [Nt] rows of each rung's window
    bool complete;                  // false: a row of a window was missing (nothing else is to be believed then)
  };
  // MH_chain::get_state_idx with Nzero = 0: row Ninit + i / add_every_N, Ninit the rows initialize(n) put in front (n of them).
  // The ring's numbering is Ninit = 1 whatever n was: the start state is row 0, further initial draws are kept in front of it.  The
  // reference's own windows on ladders initialised with 1, 3 and 5 rows (tests/golden/evidence.json.gz) are those of raw row = ring
  // row + Ninit - 1 and never reach a row in front of Ninit, so the initial rows do not enter the evidence.
  static long long state_idx(long long i, long long Nhist, int add_every_N, int Ninit = 1) {
    if (i < 0 || i >= Nhist) i = Nhist - 1;
    return Ninit + i / add_every_N;
  }
  static void window(long long Nhist, int ilen, int add_every_N, long long& first, long long& last, int Ninit = 1) {
    first = state_idx(Nhist - ilen, Nhist, add_every_N, Ninit);
    last = state_idx(Nhist, Nhist, add_every_N, Ninit);
  }
  // one ladder: Nhist[Nt] add_state calls and beta[Nt] current inverse temperatures of its chains; with Ninit != 1 the reader is
  // asked for the reference's raw rows
  static result estimate(int Nt, int add_every_N, int ilen, const long long* Nhist, const double* beta, const reader& read, int Ninit = 1) {
    result r;
    r.up.assign(Nt > 1 ? Nt - 1 : 0, 0.0); r.down = r.up; r.count.assign(Nt, 0); r.complete = true; r.evidence = 0;
    auto ratio = [&](int ia, int ib) {
      long long first, last;
      window(Nhist[ib], ilen, add_every_N, first, last, Ninit);
      const double amb = beta[ia] - beta[ib];
      double sum = 0, count = 0;
      for (long long row = first; row < last; row++) {
        double ll = 0;
        if (!read(ib, row, ll)) r.complete = false;
        volatile double x = ll * amb;   // (the product rounded before the sum, whatever the compiler's contraction rule)
        sum += x;
        count++;
      }
      r.count[ib] = (int)count;
      return sum / count;
    };
    for (int i = 0; i < Nt - 1; i++) {
      r.up[i] = ratio(i, i + 1);
      r.down[i] = -ratio(i + 1, i);
      r.evidence += (r.up[i] + r.down[i]) / 2.0;
    }
    if (Nt > 1) r.evidence += (r.up[Nt - 2] + r.down[Nt - 2]) / 2.0 / (beta[Nt - 2] / beta[Nt - 1] - 1);
    return r;
  }
};

// ---- split R-hat across independent chains ----------------------------------------------------------------------------------------
// rhat_estimator: do W independent replicas of one chain agree with each other?  The Gelman-Rubin diagnostic on split chains (Gelman
// et al., "Bayesian Data Analysis", 3rd ed., sec. 11.4), on plain rows.  The reference runs one ladder and has no counterpart.
//   * chain w's window is its own newest nrows saved rows (nrows even, >= 4), newest_w = 1 + (Nhist_w - 1) / add_every_N in the ring's
//     numbering (row 0 the start state, never part of a window): rows newest_w - nrows + 1 .. newest_w in ascending order;
//   * its first and second half, n = nrows / 2 rows each, are sequences 2w and 2w + 1: m = 2W sequences;
//   * per sequence k and feature, in row order: mean_k = (sum x) / n, then in a second walk over the same rows
//     var_k = (sum (x - mean_k) * (x - mean_k)) / (n - 1)  (two passes: a series far from zero loses nothing);
//   * per feature, over k = 0 .. m - 1 in order: M = (sum mean_k) / m, between = n * (sum (mean_k - M)^2) / (m - 1),
//     within = (sum var_k) / m, var_plus = ((n - 1) / n) * within + between / n, rhat = sqrt(var_plus / within).
// A constant feature gives the formula's IEEE result (NaN or infinity).  The engine's kernels run the same operations in the same
// order on the device's own ring (ptm_rhat): same bits.
class rhat_estimator {
 public:
  // the features of saved row `row` (the ring's numbering) of chain `chain`; false: the row is not there any more
  typedef std::function<bool(int chain, long long row, std::vector<double>& features)> reader;
  struct result {
    std::vector<double> rhat, mean, within, between;   // [nfeat]
    std::vector<double> seq_mean, seq_var;             // [2W * nfeat]: sequence k, feature f at k * nfeat + f
    bool complete;                                     // false: a row of a window was missing (nothing else is to be believed then)
    int worst() const {                                // the feature that decides: the first NaN if there is one, else the largest rhat
      int at = 0;
      for (size_t f = 0; f < rhat.size(); f++) {
        if (rhat[f] != rhat[f]) return (int)f;
        if (rhat[f] > rhat[(size_t)at]) at = (int)f;
      }
      return at;
    }
  };
  static long long newest_row(long long Nhist, int add_every_N, int first_row = 1) { return first_row + (Nhist - 1) / add_every_N; }
  // the second half of the definition, from the sequences' means and variances (r.seq_mean, r.seq_var)
  static void combine(result& r, int m, int nfeat, int n) {
    const double nd = (double)n, md = (double)m;
    r.rhat.assign((size_t)nfeat, 0.0); r.mean = r.rhat; r.within = r.rhat; r.between = r.rhat;
    for (int f = 0; f < nfeat; f++) {
      double msum = 0;
      for (int k = 0; k < m; k++) msum += r.seq_mean[(size_t)k * nfeat + f];
      const double M = msum / md;
      double bsum = 0, wsum = 0;
      for (int k = 0; k < m; k++) {
        const double d = r.seq_mean[(size_t)k * nfeat + f] - M;
        volatile double dd = d * d;   // (the product rounded before the sum, whatever the compiler's contraction rule)
        bsum += dd;
      }
      for (int k = 0; k < m; k++) wsum += r.seq_var[(size_t)k * nfeat + f];
      volatile double nb = nd * bsum;
      const double between = nb / (md - 1.0), within = wsum / md;
      volatile double scaled = ((nd - 1.0) / nd) * within;
      const double var_plus = scaled + between / nd;
      r.mean[(size_t)f] = M; r.within[(size_t)f] = within; r.between[(size_t)f] = between;
      r.rhat[(size_t)f] = std::sqrt(var_plus / within);
    }
  }
  // W chains; newest[W]: each chain's newest saved row
  static result estimate(int W, int nfeat, int nrows, const long long* newest, const reader& read) {
    result r;
    const int n = nrows / 2, m = 2 * W;
    r.complete = true;
    r.seq_mean.assign((size_t)m * nfeat, 0.0); r.seq_var = r.seq_mean;
    std::vector<double> rows((size_t)nrows * nfeat), v;
    for (int w = 0; w < W; w++) {
      for (int i = 0; i < nrows; i++) {
        if (!read(w, newest[w] - nrows + 1 + i, v) || (int)v.size() < nfeat) { r.complete = false; v.assign((size_t)nfeat, 0.0); }
        for (int f = 0; f < nfeat; f++) rows[(size_t)i * nfeat + f] = v[(size_t)f];
      }
      for (int half = 0; half < 2; half++)
        for (int f = 0; f < nfeat; f++) {
          const double* x = rows.data() + (size_t)half * n * nfeat + f;
          double sum = 0;
          for (int i = 0; i < n; i++) sum += x[(size_t)i * nfeat];
          const double mean = sum / (double)n;
          double ssq = 0;
          for (int i = 0; i < n; i++) {
            const double d = x[(size_t)i * nfeat] - mean;
            volatile double dd = d * d;
            ssq += dd;
          }
          const size_t o = (size_t)(2 * w + half) * nfeat + f;
          r.seq_mean[o] = mean;
          r.seq_var[o] = ssq / (double)(n - 1);
        }
    }
    combine(r, m, nfeat, n);
    return r;
  }
};

// ---- pooled posterior mean and covariance across independent chains -----------------------------------------------------------------
// moments_estimator: what the posterior is -- the mean and the covariance of the first nfeat parameters, pooled over W independent
// replicas of one chain, on plain rows.  The reference's write_covariance / read_covariance are empty (ptmcmc.cc:761-768).
//   * chain w's window is its own newest nrows saved rows (nrows >= 1) in ascending order, rhat_estimator's rule; N = W nrows >= 2;
//   * group = 64 chains form a block: block b holds chains 64 b .. min(64 b + 63, W - 1);
//   * s_w[f] = sum over the window's rows of x[f], S_b[f] = sum over the block's chains of s_w[f], S[f] = sum over the blocks of
//     S_b[f], mean[f] = S[f] / N;
//   * for each pair i <= j with d_i = x[i] - mean[i], in a second walk over the same rows: c_w[i,j] = sum over the rows of d_i * d_j,
//     C_b[i,j] = sum over the block's chains, C[i,j] = sum over the blocks, cov[i,j] = cov[j,i] = C[i,j] / (N - 1);
//   * every sum sequential, in that order; a constant feature gives an exact zero row and column.
// The engine's kernels run the same operations in the same order on the device's own ring (ptm_moments): same bits.
class moments_estimator {
 public:
  typedef rhat_estimator::reader reader;
  enum { group = 64 };
  struct result {
    int nfeat;
    long long count;                        // N
    std::vector<double> mean, var;          // [nfeat]; var: the diagonal of cov
    std::vector<double> cov;                // [nfeat * nfeat], row-major, both triangles (empty: not asked for)
    std::vector<double> walker_sum;         // [W * nfeat]: s_w
    bool complete;                          // false: a row of a window was missing (nothing else is to be believed then)
  };
  // W chains; newest[W]: each chain's newest saved row.  want_cov false: the mean and the variances (the diagonal pairs) alone
  static result estimate(int W, int nfeat, int nrows, const long long* newest, const reader& read, bool want_cov = true) {
    result r;
    r.nfeat = nfeat; r.count = (long long)W * nrows; r.complete = true;
    const size_t F = (size_t)nfeat, P = want_cov ? F * (F + 1) / 2 : F;
    const double Nd = (double)r.count, N1 = (double)(r.count - 1);
    r.walker_sum.assign((size_t)W * F, 0.0);
    r.mean.assign(F, 0.0); r.var = r.mean;
    std::vector<double> v, total(F, 0.0), block(F);
    auto row = [&](int w, int i) {   // row i of chain w's window into v
      if (!read(w, newest[w] - nrows + 1 + i, v) || v.size() < F) { r.complete = false; v.assign(F, 0.0); }
    };
    for (int w0 = 0; w0 < W; w0 += group) {
      block.assign(F, 0.0);
      for (int w = w0; w < W && w < w0 + group; w++) {
        double* s = r.walker_sum.data() + (size_t)w * F;
        for (int i = 0; i < nrows; i++) {
          row(w, i);
          for (size_t f = 0; f < F; f++) s[f] += v[f];
        }
        for (size_t f = 0; f < F; f++) block[f] += s[f];
      }
      for (size_t f = 0; f < F; f++) total[f] += block[f];
    }
    for (size_t f = 0; f < F; f++) r.mean[f] = total[f] / Nd;
    // the pairs along the rows of the upper triangle: (0,0) (0,1) .. (0,F-1) (1,1) ..; without the covariance the diagonal alone
    std::vector<double> d(F), cw(P), cb(P), c(P, 0.0);
    for (int w0 = 0; w0 < W; w0 += group) {
      cb.assign(P, 0.0);
      for (int w = w0; w < W && w < w0 + group; w++) {
        cw.assign(P, 0.0);
        for (int i = 0; i < nrows; i++) {
          row(w, i);
          for (size_t f = 0; f < F; f++) d[f] = v[f] - r.mean[f];
          size_t p = 0;
          for (size_t a = 0; a < F; a++)
            for (size_t b = a; b < (want_cov ? F : a + 1); b++, p++) {
              volatile double dd = d[a] * d[b];   // (the product rounded before the sum, whatever the compiler's contraction rule)
              cw[p] += dd;
            }
        }
        for (size_t p = 0; p < P; p++) cb[p] += cw[p];
      }
      for (size_t p = 0; p < P; p++) c[p] += cb[p];
    }
    if (want_cov) {
      r.cov.assign(F * F, 0.0);
      size_t p = 0;
      for (size_t a = 0; a < F; a++)
        for (size_t b = a; b < F; b++, p++) r.cov[a * F + b] = r.cov[b * F + a] = c[p] / N1;
      for (size_t f = 0; f < F; f++) r.var[f] = r.cov[f * F + f];
    } else
      for (size_t f = 0; f < F; f++) r.var[f] = c[f] / N1;
    return r;
  }
};

// ---- the covariance file (--covariance_out writes it, --covariance_file reads it) ---------------------------------------------------
// Text.  "#" lines in front: the dimension, N and replicas x rows, then the parameter names; one line with the D means; D lines with
// the rows of the D x D matrix.  Every number with 17 significant digits: reading it back gives the bits that were written.
struct covariance_data {
  int dim = 0;
  std::vector<double> mean, cov;   // [dim], [dim * dim] row-major
};
inline void write_covariance(const std::string& file, const std::vector<double>& mean, const std::vector<double>& cov, long long count, int replicas, int rows,
                             const std::vector<std::string>& names) {
  const size_t D = mean.size();
  if (cov.size() != D * D) { std::cout << "write_covariance: the matrix must be " << D << " x " << D << std::endl; exit(1); }
  std::ofstream out(file.c_str());
  out << "# posterior moments: dim " << D << " N " << count << " replicas " << replicas << " x rows " << rows << "\n# parameters:";
  for (size_t i = 0; i < names.size(); i++) out << " " << names[i];
  out << "\n";
  char buf[40];
  for (size_t i = 0; i < D; i++) { snprintf(buf, sizeof buf, "%.17g", mean[i]); out << (i ? " " : "") << buf; }
  out << "\n";
  for (size_t i = 0; i < D; i++) {
    for (size_t j = 0; j < D; j++) { snprintf(buf, sizeof buf, "%.17g", cov[i * D + j]); out << (j ? " " : "") << buf; }
    out << "\n";
  }
  out.close();
  if (!out) { std::cout << "write_covariance: cannot write '" << file << "'" << std::endl; exit(1); }
}
// refuses, with a message and exit(1): a missing file, another dimension than `dim`, a value that is not a finite number, too few or
// too many values, a matrix that is not symmetric
inline covariance_data read_covariance(const std::string& file, int dim) {
  auto refuse = [&](const std::string& why) { std::cout << "read_covariance: '" << file << "': " << why << std::endl; exit(1); };
  std::ifstream in(file.c_str());
  if (!in) refuse("cannot open the file");
  std::vector<std::vector<double> > lines;
  std::string line;
  while (std::getline(in, line)) {
    const size_t at = line.find_first_not_of(" \t\r");
    if (at == std::string::npos || line[at] == '#') continue;
    std::vector<double> vals;
    const char* p = line.c_str() + at;
    while (*p) {
      char* end = nullptr;
      const double x = strtod(p, &end);
      if (end == p) refuse("not a number: '" + std::string(p).substr(0, 20) + "'");
      if (!(x - x == 0)) refuse("a value is not finite");
      vals.push_back(x);
      p = end;
      while (*p == ' ' || *p == '\t' || *p == '\r') p++;
    }
    lines.push_back(vals);
  }
  if (lines.empty() || (int)lines[0].size() != dim) {
    std::ostringstream ss; ss << "the mean line holds " << (lines.empty() ? 0 : lines[0].size()) << " values; the parameter space has " << dim;
    refuse(ss.str());
  }
  if ((int)lines.size() != dim + 1) { std::ostringstream ss; ss << "expected " << dim << " matrix rows, found " << lines.size() - 1; refuse(ss.str()); }
  covariance_data c;
  c.dim = dim; c.mean = lines[0];
  for (int i = 0; i < dim; i++) {
    if ((int)lines[(size_t)i + 1].size() != dim) { std::ostringstream ss; ss << "matrix row " << i << " holds " << lines[(size_t)i + 1].size() << " values, not " << dim; refuse(ss.str()); }
    c.cov.insert(c.cov.end(), lines[(size_t)i + 1].begin(), lines[(size_t)i + 1].end());
  }
  for (int i = 0; i < dim; i++)
    for (int j = 0; j < i; j++)
      if (c.cov[(size_t)i * dim + j] != c.cov[(size_t)j * dim + i]) { std::ostringstream ss; ss << "the matrix is not symmetric at (" << i << "," << j << ")"; refuse(ss.str()); }
  return c;
}

// ---- exact pooled quantiles across independent chains --------------------------------------------------------------------------------
// quantile_estimator: the median and the credible interval of each of the first nfeat parameters, pooled over W independent
// replicas of one chain, on plain rows.  The reference writes no quantiles.
//   * chain w's window is its own newest nrows saved rows (nrows >= 1), rhat_estimator's rule; the sample of a feature is the
//     N = W nrows values of the windows (N >= 1: a single sample is its own every quantile);
//   * values are ordered by the 64-bit key  u ^ (u >> 63 ? ~0 : 1 << 63)  of their bit pattern u: the order of the reals, -0 before
//     +0, -inf / +inf at the ends; sorted: s_0 <= ... <= s_{N-1};
//   * for a probability p in [0, 1]:  h = (double)(N - 1) * p,  lo = floor(h),  hi = min(lo + 1, N - 1),  g = h - lo,
//     q = (g == 0) ? s_lo : s_lo + g * (s_hi - s_lo)  (multiply, then add): the linear rule, numpy's default (Hyndman and Fan
//     type 7); x_lo = s_lo and x_hi = s_hi beside it.  Nothing is special-cased.
// The engine's kernels select the same order statistics by radix digits on the device's own ring (ptm_quantiles): an order
// statistic is a value of the sample, so the bits are the same.
class quantile_estimator {
 public:
  typedef rhat_estimator::reader reader;
  struct result {
    int nfeat;
    long long count;                   // N
    std::vector<double> probs;         // [nq]
    std::vector<double> q, x_lo, x_hi; // [nq * nfeat], [k * nfeat + f]
    bool complete;                     // false: a row of a window was missing (nothing else is to be believed then)
  };
  static uint64_t key(double x) { uint64_t u; memcpy(&u, &x, 8); return u ^ ((u >> 63) ? ~(uint64_t)0 : ((uint64_t)1 << 63)); }
  static double value(uint64_t k) { const uint64_t u = k ^ ((k >> 63) ? ((uint64_t)1 << 63) : ~(uint64_t)0); double x; memcpy(&x, &u, 8); return x; }
  // q, x_lo, x_hi [probs.size()] of one sample (keys: sorted here)
  static void of_sample(std::vector<uint64_t>& keys, const std::vector<double>& probs, double* q, double* x_lo, double* x_hi, size_t stride = 1) {
    std::sort(keys.begin(), keys.end());
    const long long N = (long long)keys.size();
    for (size_t k = 0; k < probs.size(); k++) {
      const double h = (double)(N - 1) * probs[k], fl = std::floor(h), g = h - fl;
      const long long lo = (long long)fl, hi = std::min(lo + 1, N - 1);
      const double a = value(keys[(size_t)lo]), c = value(keys[(size_t)hi]);
      volatile double step = g * (c - a);   // (the product rounded before the sum, whatever the compiler's contraction rule)
      q[k * stride] = g == 0 ? a : a + step;
      x_lo[k * stride] = a;
      x_hi[k * stride] = c;
    }
  }
  // W chains; newest[W]: each chain's newest saved row
  static result estimate(int W, int nfeat, int nrows, const long long* newest, const reader& read, const std::vector<double>& probs) {
    result r;
    r.nfeat = nfeat; r.count = (long long)W * nrows; r.complete = true; r.probs = probs;
    const size_t F = (size_t)nfeat, Q = probs.size(), N = (size_t)r.count;
    r.q.assign(Q * F, 0.0); r.x_lo = r.q; r.x_hi = r.q;
    std::vector<uint64_t> keys(N * F);   // [f * N + sample]
    std::vector<double> v;
    size_t at = 0;
    for (int w = 0; w < W; w++)
      for (int i = 0; i < nrows; i++, at++) {
        if (!read(w, newest[w] - nrows + 1 + i, v) || v.size() < F) { r.complete = false; v.assign(F, 0.0); }
        for (size_t f = 0; f < F; f++) keys[f * N + at] = key(v[f]);
      }
    std::vector<uint64_t> one(N);
    for (size_t f = 0; f < F; f++) {
      one.assign(keys.begin() + f * N, keys.begin() + (f + 1) * N);
      of_sample(one, probs, r.q.data() + f, r.x_lo.data() + f, r.x_hi.data() + f, F);
    }
    return r;
  }
};

// ---- the quantile file (--quantiles_out writes it) -----------------------------------------------------------------------------------
// Text.  One "#" line in front: the dimension, N, replicas x rows and the probabilities; then one line per parameter: its name and
// its quantile at each probability.  Every number with 17 significant digits: reading it back gives the bits that were written.
struct quantiles_data {
  int dim = 0;
  long long count = 0;
  int replicas = 0, rows = 0;
  std::vector<double> probs, q;   // [nq], [nq * dim] as quantile_estimator::result::q
  std::vector<std::string> names;
};
inline void write_quantiles(const std::string& file, const quantile_estimator::result& r, int replicas, int rows, const std::vector<std::string>& names) {
  const size_t D = (size_t)r.nfeat, Q = r.probs.size();
  if (r.q.size() != Q * D || names.size() != D) { std::cout << "write_quantiles: " << Q << " quantiles of " << D << " named parameters are needed" << std::endl; exit(1); }
  for (size_t i = 0; i < D; i++)
    if (names[i].empty() || names[i].find_first_of(" \t\r\n#") != std::string::npos) { std::cout << "write_quantiles: parameter name '" << names[i] << "' must be one word without '#'" << std::endl; exit(1); }
  std::ofstream out(file.c_str());
  char buf[40];
  out << "# posterior quantiles: dim " << D << " N " << r.count << " replicas " << replicas << " x rows " << rows << " probs";
  for (size_t k = 0; k < Q; k++) { snprintf(buf, sizeof buf, "%.17g", r.probs[k]); out << " " << buf; }
  out << "\n";
  for (size_t i = 0; i < D; i++) {
    out << names[i];
    for (size_t k = 0; k < Q; k++) { snprintf(buf, sizeof buf, "%.17g", r.q[k * D + i]); out << " " << buf; }
    out << "\n";
  }
  out.close();
  if (!out) { std::cout << "write_quantiles: cannot write '" << file << "'" << std::endl; exit(1); }
}
// refuses, with a message and exit(1): a missing file, a missing or malformed header, a probability outside [0, 1], another number
// of parameter lines than the header's dimension, a line with too few or too many values, a value that is not a number (an
// infinite quantile is a value like any other; a NaN is refused)
inline quantiles_data read_quantiles(const std::string& file) {
  auto refuse = [&](const std::string& why) { std::cout << "read_quantiles: '" << file << "': " << why << std::endl; exit(1); };
  std::ifstream in(file.c_str());
  if (!in) refuse("cannot open the file");
  quantiles_data d;
  std::string line, word;
  if (!std::getline(in, line)) refuse("the file is empty");
  {
    std::istringstream ss(line);
    std::string w[4];
    if (!(ss >> w[0] >> w[1] >> w[2] >> w[3]) || w[0] != "#" || w[1] != "posterior" || w[2] != "quantiles:" || w[3] != "dim") refuse("the header line is missing");
    std::string sN, srep, sx, srows, sprobs;
    if (!(ss >> d.dim >> sN >> d.count >> srep >> d.replicas >> sx >> srows >> d.rows >> sprobs) || sN != "N" || srep != "replicas" || sx != "x" || srows != "rows" || sprobs != "probs" || d.dim < 1)
      refuse("the header line is malformed");
    while (ss >> word) {
      char* end = nullptr;
      const double p = strtod(word.c_str(), &end);
      if (end == word.c_str() || *end) refuse("not a number: '" + word + "'");
      if (!(p >= 0.0 && p <= 1.0)) refuse("a probability is outside [0, 1]");
      d.probs.push_back(p);
    }
    if (d.probs.empty()) refuse("the header names no probability");
  }
  const size_t Q = d.probs.size();
  std::vector<std::vector<double> > rows;
  while (std::getline(in, line)) {
    const size_t at = line.find_first_not_of(" \t\r");
    if (at == std::string::npos || line[at] == '#') continue;
    std::istringstream ss(line);
    std::string name;
    ss >> name;
    std::vector<double> vals;
    while (ss >> word) {
      char* end = nullptr;
      const double x = strtod(word.c_str(), &end);
      if (end == word.c_str() || *end) refuse("not a number: '" + word + "'");
      if (x != x) refuse("a value is not a number");
      vals.push_back(x);
    }
    if (vals.size() != Q) { std::ostringstream m; m << "the line of '" << name << "' holds " << vals.size() << " values, not " << Q; refuse(m.str()); }
    d.names.push_back(name);
    rows.push_back(vals);
  }
  if ((int)rows.size() != d.dim) { std::ostringstream m; m << "expected " << d.dim << " parameter lines, found " << rows.size(); refuse(m.str()); }
  d.q.assign(Q * (size_t)d.dim, 0.0);
  for (size_t i = 0; i < rows.size(); i++)
    for (size_t k = 0; k < Q; k++) d.q[k * (size_t)d.dim + i] = rows[i][k];
  return d;
}

// ---- corner-plot histograms across independent chains -----------------------------------------------------------------------------------
// histogram_estimator: the counts of a corner plot -- the 1-D histogram of each of the first nfeat parameters and the 2-D histogram
// of each pair of them -- pooled over W independent replicas of one chain, on plain rows.  The reference bins on the host with numpy
// (python/corner_with_covar.py: np.histogram, np.histogram2d); these are numpy's counts.
//   * chain w's window is its own newest nrows saved rows (nrows >= 1), rhat_estimator's rule; the sample is the N = W nrows rows
//     of the windows (quantile_estimator's sample);
//   * the edges of feature f, lo < hi:  step = (hi - lo) / (double)nbins,  edge_k = lo + (double)k * step  (multiply, then add) for
//     k < nbins,  edge_nbins = hi: np.linspace(lo, hi, nbins + 1) bit for bit.  They must be finite and strictly increasing;
//   * x lies in bin k iff edge_k <= x < edge_{k+1} (std::upper_bound on the edges), the last bin closed: x == hi lies in bin
//     nbins - 1; -0.0 compares as 0; x < lo counts as below, x > hi as above, a NaN as neither;
//   * h1[f * nbins + k]: the samples of feature f in bin k;  h2[(p * nbins + ki) * nbins + kj]: the rows whose feature i lies in bin
//     ki and whose feature j in bin kj, pairs i < j in row-major order, p = i nfeat - i (i + 1) / 2 + (j - i - 1); a row with either
//     value outside its range is left out of that pair only.
// The engine's kernels count the same on the device's own ring (ptm_histograms): integers, so the same to the last unit.  Counts of
// walker splits with the same lo, hi and nbins simply add.
class histogram_estimator {
 public:
  typedef rhat_estimator::reader reader;
  struct result {
    int nfeat = 0, nbins = 0;
    long long count = 0;               // N
    std::vector<double> lo, hi;        // [nfeat]
    std::vector<int64_t> h1, h2;       // [nfeat * nbins], [npairs * nbins * nbins] (empty: no pairs were asked for)
    std::vector<int64_t> below, above; // [nfeat]
    bool complete = true;              // false: a row of a window was missing (nothing else is to be believed then)
  };
  enum { BELOW = -1, ABOVE = -2, NOT_A_NUMBER = -3 };
  static std::vector<double> edges(double lo, double hi, int nbins) {
    std::vector<double> e((size_t)nbins + 1);
    const double step = (hi - lo) / (double)nbins;
    for (int k = 0; k < nbins; k++) {
      volatile double up = (double)k * step;   // (the product rounded before the sum, whatever the compiler's contraction rule)
      e[(size_t)k] = lo + up;
    }
    e[(size_t)nbins] = hi;
    return e;
  }
  // finite, lo < hi, strictly increasing: what a range must give to hold nbins bins
  static bool edges_ok(double lo, double hi, int nbins) {
    if (!(std::isfinite(lo) && std::isfinite(hi) && lo < hi) || nbins < 1) return false;
    const std::vector<double> e = edges(lo, hi, nbins);
    for (size_t k = 0; k + 1 < e.size(); k++)
      if (!(std::isfinite(e[k]) && e[k] < e[k + 1])) return false;
    return true;
  }
  // the bin of x among nbins + 1 edges, or BELOW, ABOVE, NOT_A_NUMBER
  static int bin(const std::vector<double>& e, double x) {
    const int nbins = (int)e.size() - 1;
    if (x != x) return NOT_A_NUMBER;
    if (x < e[0]) return BELOW;
    if (x > e[(size_t)nbins]) return ABOVE;
    if (x == e[(size_t)nbins]) return nbins - 1;
    return (int)(std::upper_bound(e.begin(), e.end(), x) - e.begin()) - 1;
  }
  static size_t npairs(int nfeat) { return (size_t)nfeat * (size_t)(nfeat - 1) / 2; }
  static size_t pair_index(int nfeat, int i, int j) { return (size_t)i * nfeat - (size_t)i * (i + 1) / 2 + (size_t)(j - i - 1); }
  // W chains; newest[W]: each chain's newest saved row.  Every range must pass edges_ok.
  static result estimate(int W, int nfeat, int nrows, const long long* newest, const reader& read, const std::vector<double>& lo, const std::vector<double>& hi,
                         int nbins, bool pairs = true) {
    result r;
    r.nfeat = nfeat; r.nbins = nbins; r.count = (long long)W * nrows; r.lo = lo; r.hi = hi;
    const size_t F = (size_t)nfeat, B = (size_t)nbins;
    r.h1.assign(F * B, 0); r.below.assign(F, 0); r.above.assign(F, 0);
    if (pairs) r.h2.assign(npairs(nfeat) * B * B, 0);
    std::vector<std::vector<double> > e;
    for (size_t f = 0; f < F; f++) e.push_back(edges(lo[f], hi[f], nbins));
    std::vector<double> v;
    std::vector<int> k(F);
    for (int w = 0; w < W; w++)
      for (int i = 0; i < nrows; i++) {
        if (!read(w, newest[w] - nrows + 1 + i, v) || v.size() < F) { r.complete = false; continue; }
        for (size_t f = 0; f < F; f++) {
          k[f] = bin(e[f], v[f]);
          if (k[f] >= 0) r.h1[f * B + (size_t)k[f]]++;
          else if (k[f] == BELOW) r.below[f]++;
          else if (k[f] == ABOVE) r.above[f]++;
        }
        if (!pairs) continue;
        size_t p = 0;
        for (size_t a = 0; a < F; a++)
          for (size_t b = a + 1; b < F; b++, p++)
            if (k[a] >= 0 && k[b] >= 0) r.h2[(p * B + (size_t)k[a]) * B + (size_t)k[b]]++;
      }
    return r;
  }
};

// ---- the corner file (--corner_out writes it) ---------------------------------------------------------------------------------------------
// Text.  One "#" line in front: the dimension, the bins, N, the replicas, the rows and the number of pair lines; then one line per
// parameter: its name, lo, hi, below, above and its nbins counts; then one line per pair i < j, in row-major order: the two names
// and the nbins * nbins counts, the first parameter's bin the slower index.  Doubles with 17 significant digits: reading them back
// gives the bits that were written.
struct corner_data {
  int dim = 0, nbins = 0;
  long long count = 0;
  int replicas = 0, rows = 0;
  std::vector<std::string> names;
  histogram_estimator::result hist;   // lo, hi, h1, h2, below, above
};
inline void write_corner(const std::string& file, const histogram_estimator::result& r, int replicas, int rows, const std::vector<std::string>& names) {
  const size_t D = (size_t)r.nfeat, B = (size_t)r.nbins, P = r.h2.empty() ? 0 : histogram_estimator::npairs(r.nfeat);
  if (r.nfeat < 1 || r.nbins < 1 || r.h1.size() != D * B || r.h2.size() != P * B * B || r.lo.size() != D || r.hi.size() != D || r.below.size() != D || r.above.size() != D || names.size() != D) {
    std::cout << "write_corner: " << B << " bins of " << D << " named parameters and of their pairs are needed" << std::endl; exit(1);
  }
  for (size_t i = 0; i < D; i++)
    if (names[i].empty() || names[i].find_first_of(" \t\r\n#") != std::string::npos) { std::cout << "write_corner: parameter name '" << names[i] << "' must be one word without '#'" << std::endl; exit(1); }
  std::ofstream out(file.c_str());
  char buf[40];
  out << "# posterior histograms: dim " << D << " nbins " << B << " N " << r.count << " replicas " << replicas << " rows " << rows << " pairs " << P << "\n";
  for (size_t i = 0; i < D; i++) {
    out << names[i];
    snprintf(buf, sizeof buf, "%.17g", r.lo[i]); out << " " << buf;
    snprintf(buf, sizeof buf, "%.17g", r.hi[i]); out << " " << buf;
    out << " " << r.below[i] << " " << r.above[i];
    for (size_t k = 0; k < B; k++) out << " " << r.h1[i * B + k];
    out << "\n";
  }
  if (P) {
    size_t p = 0;
    for (size_t i = 0; i < D; i++)
      for (size_t j = i + 1; j < D; j++, p++) {
        out << names[i] << " " << names[j];
        for (size_t k = 0; k < B * B; k++) out << " " << r.h2[p * B * B + k];
        out << "\n";
      }
  }
  out.close();
  if (!out) { std::cout << "write_corner: cannot write '" << file << "'" << std::endl; exit(1); }
}
// refuses, with a message and exit(1): a missing file, a missing or malformed header, bins outside 1..128, another number of
// parameter or pair lines than the header's, a line with too few or too many values, a range that is not two finite numbers with
// lo < hi, a count that is not a non-negative whole number
inline corner_data read_corner(const std::string& file) {
  auto refuse = [&](const std::string& why) { std::cout << "read_corner: '" << file << "': " << why << std::endl; exit(1); };
  std::ifstream in(file.c_str());
  if (!in) refuse("cannot open the file");
  corner_data d;
  std::string line, word;
  if (!std::getline(in, line)) refuse("the file is empty");
  long long P = 0;
  {
    std::istringstream ss(line);
    std::string w[4];
    if (!(ss >> w[0] >> w[1] >> w[2] >> w[3]) || w[0] != "#" || w[1] != "posterior" || w[2] != "histograms:" || w[3] != "dim") refuse("the header line is missing");
    std::string sb, sN, srep, srows, sp;
    if (!(ss >> d.dim >> sb >> d.nbins >> sN >> d.count >> srep >> d.replicas >> srows >> d.rows >> sp >> P) || sb != "nbins" || sN != "N" || srep != "replicas" || srows != "rows" || sp != "pairs" || d.dim < 1 || (ss >> word))
      refuse("the header line is malformed");
    if (d.nbins < 1 || d.nbins > 128) refuse("the bins are outside 1..128");
    if (P != 0 && P != (long long)histogram_estimator::npairs(d.dim)) refuse("the pairs are not those of the dimension");
  }
  const size_t D = (size_t)d.dim, B = (size_t)d.nbins;
  histogram_estimator::result& r = d.hist;
  r.nfeat = d.dim; r.nbins = d.nbins; r.count = d.count;
  auto count_of = [&](const std::string& text) {
    char* end = nullptr;
    errno = 0;
    const long long c = strtoll(text.c_str(), &end, 10);
    if (end == text.c_str() || *end || errno || c < 0) refuse("not a count: '" + text + "'");
    return (int64_t)c;
  };
  auto number_of = [&](const std::string& text) {
    char* end = nullptr;
    const double x = strtod(text.c_str(), &end);
    if (end == text.c_str() || *end) refuse("not a number: '" + text + "'");
    if (!std::isfinite(x)) refuse("an end of a range is not finite");
    return x;
  };
  size_t lines = 0;
  while (std::getline(in, line)) {
    const size_t at = line.find_first_not_of(" \t\r");
    if (at == std::string::npos || line[at] == '#') continue;
    std::istringstream ss(line);
    std::vector<std::string> words;
    while (ss >> word) words.push_back(word);
    if (lines < D) {
      if (words.size() != 5 + B) { std::ostringstream m; m << "the line of '" << words[0] << "' holds " << words.size() << " words, not " << 5 + B; refuse(m.str()); }
      d.names.push_back(words[0]);
      r.lo.push_back(number_of(words[1]));
      r.hi.push_back(number_of(words[2]));
      if (!(r.lo.back() < r.hi.back())) refuse("a range is not lo < hi");
      r.below.push_back(count_of(words[3]));
      r.above.push_back(count_of(words[4]));
      for (size_t k = 0; k < B; k++) r.h1.push_back(count_of(words[5 + k]));
    } else {
      if (words.size() != 2 + B * B) { std::ostringstream m; m << "the line of pair '" << words[0] << "' holds " << words.size() << " words, not " << 2 + B * B; refuse(m.str()); }
      for (size_t k = 0; k < B * B; k++) r.h2.push_back(count_of(words[2 + k]));
    }
    lines++;
  }
  if (lines != D + (size_t)P) { std::ostringstream m; m << "expected " << D << " parameter lines and " << P << " pair lines, found " << lines; refuse(m.str()); }
  return d;
}

// ---- the statistics of the proposal test (test_proposal.hh:350-502, 592-644) ------------------------------------------------------
// kl_estimator: the k-NN Kullback-Leibler estimator of Perez-Cruz with k = 1 and the Gaussian "fake KL" from means and covariances,
// on plain rows (sample i of a set at x + i * dim), as test_proposal states them with approx_nn = false.
//   * dist2 is state::dist2 (states.cc:207-233): per dimension diff = |b - a|; in a wrapped dimension also the alternative, both
//     points shifted down by half the domain and wrap-enforced (boundary::enforce above), the smaller of the two; diff * diff is
//     summed in dimension order, the product rounded before it is added;
//   * all_nnd2: for every point the nearest OTHER INDEX of its own set (a duplicate gives 0); one_nnd2: the nearest point of Q;
//   * kl: r = all_nnd2(P), s[i] = one_nnd2(P[i], Q); the floor is element kfloor + 1 = 6 of the sorted r and is applied to both;
//     result = sum_i -log(r_i / s_i) in index order, result *= (0.5 * dim) / N, result += log(M / (N - 1.0)).  N < 7 or M < 1 is
//     refused (the reference reads out of bounds there);
//   * fake_kl: means and covariances sequentially in sample order, divided by N - 1; the unbiasing factor uses nQ = the size of P,
//     as the reference writes it.  The inverse and the determinant are Gauss-Jordan with partial pivoting (the reference uses Eigen's:
//     the last digits differ).
// The engine's ptm_nn_dist2 runs the two searches on the device, every pair's sum in the same order: same bits (combine() is the rest).
class kl_estimator {
 public:
  static const int kfloor = 5;
  struct result {
    double value;
    std::vector<double> r1sqs, s1sqs;   // [N] the distances within P and to Q, before the floor
  };
  // space: null, or the space whose wrapped dimensions count
  static double dist2(const double* a, const double* b, int dim, const stateSpace* space = nullptr) {
    double result = 0;
    for (int i = 0; i < dim; i++) {
      double xa = a[i], xb = b[i];
      double diff = std::fabs(xb - xa);
      if (space && space->get_bound(i).isWrapped()) {
        const boundary bd = space->get_bound(i);
        double xmin, xmax;
        bd.getDomainLimits(xmin, xmax);
        const double halfwrap = (xmax - xmin) / 2;
        xa -= halfwrap;
        xb -= halfwrap;
        bd.enforce(xa);
        bd.enforce(xb);
        const double altdiff = std::fabs(xb - xa);
        if (altdiff < diff) diff = altdiff;
      }
      volatile double dd = diff * diff;   // (the product rounded before the sum, whatever the compiler's contraction rule)
      result += dd;
    }
    return result;
  }
  static std::vector<double> all_nnd2(const double* P, long long N, int dim, const stateSpace* space = nullptr) {   // test_proposal.hh:442-464
    std::vector<double> nnd2((size_t)N, -1.0);
    for (long long i = 0; i < N; i++)
      for (long long j = i + 1; j < N; j++) {
        const double d2 = dist2(P + i * dim, P + j * dim, dim, space);
        if (nnd2[(size_t)i] < 0 || nnd2[(size_t)i] > d2) nnd2[(size_t)i] = d2;
        if (nnd2[(size_t)j] < 0 || nnd2[(size_t)j] > d2) nnd2[(size_t)j] = d2;
      }
    return nnd2;
  }
  static double one_nnd2(const double* p, const double* Q, long long M, int dim, const stateSpace* space = nullptr) {   // test_proposal.hh:424-441
    double nnd2 = -1;
    for (long long i = 0; i < M; i++) {
      const double d2 = dist2(Q + i * dim, p, dim, space);
      if (nnd2 < 0 || nnd2 > d2) nnd2 = d2;
    }
    return nnd2;
  }
  static void check_sizes(long long N, long long M) {
    if (N < kfloor + 2 || M < 1) throw std::invalid_argument("kl_estimator: needs at least 7 samples of P and 1 of Q");
  }
  // test_proposal.hh:400-421 from the two distance arrays (taken by value: the floor is applied to the copies)
  static double combine(std::vector<double> r1sqs, std::vector<double> s1sqs, int dim_, long long M) {
    const double N = (double)r1sqs.size();
    check_sizes((long long)r1sqs.size(), M);
    std::vector<double> dists = r1sqs;
    std::sort(dists.begin(), dists.end());
    const double floor = dists[kfloor + 1];
    for (auto& d2 : r1sqs) if (d2 < floor) d2 = floor;
    for (auto& d2 : s1sqs) if (d2 < floor) d2 = floor;
    double result = 0;
    for (size_t i = 0; i < r1sqs.size(); i++) result += -std::log(r1sqs[i] / s1sqs[i]);
    const double dim = dim_;
    volatile double scaled = result * ((0.5 * dim) / N);
    result = scaled;
    result += std::log((int)M / (N - 1.0));
    return result;
  }
  static result kl(const double* P, long long N, const double* Q, long long M, int dim, const stateSpace* space = nullptr) {
    check_sizes(N, M);
    result r;
    r.r1sqs = all_nnd2(P, N, dim, space);
    r.s1sqs.resize((size_t)N);
    for (long long i = 0; i < N; i++) r.s1sqs[(size_t)i] = one_nnd2(P + i * dim, Q, M, dim, space);
    r.value = combine(r.r1sqs, r.s1sqs, dim, M);
    return r;
  }
  // test_proposal.hh:592-644: mean[dim] and cov[dim * dim]
  static void sample_cov(const double* X, long long N, int dim, std::vector<double>& mean, std::vector<double>& cov) {
    mean.assign((size_t)dim, 0.0);
    cov.assign((size_t)dim * dim, 0.0);
    for (long long s = 0; s < N; s++)
      for (int j = 0; j < dim; j++) mean[(size_t)j] += X[s * dim + j];
    for (auto& x : mean) x /= (double)(size_t)N;
    for (long long s = 0; s < N; s++)
      for (int j = 0; j < dim; j++) {
        const double jdiff = X[s * dim + j] - mean[(size_t)j];
        volatile double jj = jdiff * jdiff;
        cov[(size_t)j * dim + j] += jj;
        for (int i = j + 1; i < dim; i++) {
          const double idiff = X[s * dim + i] - mean[(size_t)i];
          volatile double val = idiff * jdiff;
          cov[(size_t)i * dim + j] += val;
          cov[(size_t)j * dim + i] += val;
        }
      }
    for (auto& x : cov) x /= ((double)(size_t)N - 1.0);
  }
  // inverse [n * n] and determinant of a [n * n] by Gauss-Jordan elimination with partial pivoting; false: singular
  static bool invert(std::vector<double> a, int n, std::vector<double>& inv, double& det) {
    inv.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; i++) inv[(size_t)i * n + i] = 1.0;
    det = 1.0;
    for (int c = 0; c < n; c++) {
      int piv = c;
      for (int r = c + 1; r < n; r++)
        if (std::fabs(a[(size_t)r * n + c]) > std::fabs(a[(size_t)piv * n + c])) piv = r;
      if (a[(size_t)piv * n + c] == 0.0) { det = 0.0; return false; }
      if (piv != c) {
        for (int k = 0; k < n; k++) { std::swap(a[(size_t)piv * n + k], a[(size_t)c * n + k]); std::swap(inv[(size_t)piv * n + k], inv[(size_t)c * n + k]); }
        det = -det;
      }
      const double d = a[(size_t)c * n + c];
      det *= d;
      for (int k = 0; k < n; k++) { a[(size_t)c * n + k] /= d; inv[(size_t)c * n + k] /= d; }
      for (int r = 0; r < n; r++) {
        if (r == c) continue;
        const double f = a[(size_t)r * n + c];
        if (f == 0.0) continue;
        for (int k = 0; k < n; k++) {
          volatile double fa = f * a[(size_t)c * n + k], fi = f * inv[(size_t)c * n + k];
          a[(size_t)r * n + k] -= fa;
          inv[(size_t)r * n + k] -= fi;
        }
      }
    }
    return true;
  }
  // test_proposal.hh:466-502
  static double fake_kl(const double* P, long long N, const double* Q, long long M, int dim) {
    if (N < 2 || M < 2) throw std::invalid_argument("kl_estimator::fake_kl: needs at least 2 samples of each set");
    std::vector<double> meanP, meanQ, covP, covQ, inv, prod((size_t)dim * dim, 0.0), unscaled((size_t)dim * dim), tmp;
    sample_cov(P, N, dim, meanP, covP);
    sample_cov(Q, M, dim, meanQ, covQ);
    const int nQ = (int)N;   // (as the reference writes it: samplesP.size())
    const double unbiasing_factor = (nQ - dim - 2.0) / (nQ - 1.0);
    double det = 0;
    if (!invert(covQ, dim, inv, det)) return NAN;
    for (auto& x : inv) x *= unbiasing_factor;
    auto at = [dim](int i, int j) { return (size_t)i * dim + j; };
    double trace = 0;
    for (int i = 0; i < dim; i++)
      for (int j = 0; j < dim; j++) {
        double s = 0;
        for (int k = 0; k < dim; k++) { volatile double t = covP[at(i, k)] * inv[at(k, j)]; s += t; }
        prod[at(i, j)] = s;
        unscaled[at(i, j)] = s / unbiasing_factor;
      }
    for (int i = 0; i < dim; i++) trace += prod[at(i, i)];
    double result = 0;
    result += -dim + trace;
    double det2 = 0;
    invert(unscaled, dim, tmp, det2);
    result += -std::log(det2);
    double quad = 0;
    for (int i = 0; i < dim; i++) {
      double s = 0;
      for (int j = 0; j < dim; j++) { volatile double t = inv[at(i, j)] * (meanP[(size_t)j] - meanQ[(size_t)j]); s += t; }
      volatile double t = (meanP[(size_t)i] - meanQ[(size_t)i]) * s;
      quad += t;
    }
    result += quad - (dim + trace) / nQ;
    return 0.5 * result;
  }
};

// kl_verdict: how test_proposal::test judges a statistic against its redraws (test_proposal.hh:311-343) -- the redraw values by
// magnitude, Ncut = int(sqrt(ntry)), the cut half way between sorted entries ntry - Ncut and ntry - Ncut - 1 (none, 0, with one
// redraw), and the lines it prints; name is "KL" or "fKL" (the line after FAIL says "KL value" for both, as written there).
class kl_verdict {
 public:
  int Ncut;
  double cut_frac, cut;
  bool pass;
  kl_verdict(std::vector<double> diffs, double alt) {
    const int ntry = (int)diffs.size();
    for (auto& d : diffs) d = std::fabs(d);
    std::sort(diffs.begin(), diffs.end());
    Ncut = (int)std::sqrt((double)ntry);
    cut = 0;
    cut_frac = Ncut * 1.0 / ntry;
    if (ntry > 1) cut = (diffs[(size_t)(ntry - Ncut)] + diffs[(size_t)(ntry - Ncut - 1)]) / 2.0;
    have_cut = ntry > 1;
    pass = alt < cut;
  }
  std::string lines(const std::string& name, double transformed, double transformedX, double alt, double altX, double ncyc) const {
    std::ostringstream os;
    if (have_cut) os << "\nEstimate that only " << cut_frac * 100 << "% of " << name << "diff measurements are likely to exceed " << cut << " for matching distributions.\n";
    os << "Transformed " << name << "div=" << transformed << " <-> " << transformedX << "\n";
    os << "Alt-transformed " << name << "div=" << alt << " <-> " << altX << "\n";
    if (alt - transformed > std::fabs(cut))
      os << "When 'Transformed' is signficantly less than 'alt-Transformed' it may indicate that the effect of the proposal (after ncyc=" << ncyc
         << " applications) is too small to measure at this level.\n";
    if (pass) os << "PASS\n";
    else os << "FAIL\nKL value is " << alt / cut << " times the stated threshold.\n";
    return os.str();
  }

 private:
  bool have_cut;
};

// evidence_records: what the statistics block keeps of the totals (chain.cc:1603-1675) -- the pyramid total_evidence_records (level 0
// every total from the second epoch on; level i the average of the last two of level i-1 whenever evidence_count is a multiple of
// 2^i), the "recent ev analysis" over the newest 2 (Ndim - j) + 1 entries of each level but the top one, and the smallest standard
// error seen (1e100 until there is one: six epochs) -- and the lines it prints, as written there.
class evidence_records {
  std::vector<std::vector<double> > records;
  int evidence_count, records_dim;
  double best_stderr;

 public:
  evidence_records() : evidence_count(0), records_dim(0), best_stderr(1e100) {}
  double best() const { return best_stderr; }
  int epochs() const { return evidence_count; }
  const std::vector<std::vector<double> >& levels() const { return records; }
  // one more total; returns the lines of chain.cc:1600-1675 (default stream formatting)
  std::string push(double evidence, bool verbose_evid = true) {
    std::ostringstream os;
    os << "Total log-evidence: " << evidence << "\n";
    evidence_count++;
    int Ndim = 0;
    while ((2 << Ndim) <= evidence_count) Ndim++;   // (int)log2(evidence_count)
    if (Ndim > records_dim) { records.push_back(std::vector<double>()); records_dim++; }
    if (records_dim > 0) {   // (saved from the second epoch of every scale on)
      records[0].push_back(evidence);
      os << "total_evidence_records[0][" << evidence_count - 2 << "]=" << evidence << "\n";
    }
    for (int i = 1; i < records_dim; i++)
      if (evidence_count % (1 << i) == 0) {
        os << "i=" << i << " ec=" << evidence_count << " 1<<(i)=" << (1 << i) << " mod=" << (evidence_count % (1 << i)) << "\n";
        const int iend = (int)records[i - 1].size() - 1;
        records[i].push_back((records[i - 1][iend - 1] + records[i - 1][iend]) / 2.0);
      }
    if (Ndim > 0) {
      os << "total_log_evs:\n";
      const int ndisplaymax = verbose_evid ? 20 : -1, ntot = (int)records[0].size();
      const int ndisplay = ntot > ndisplaymax ? ndisplaymax : ntot;
      for (int i = ntot - ndisplay; i < ntot; i++) {
        for (int j = 0; j < (int)records.size(); j++) {
          const int ind = (ntot + 1) / (1 << j) + (i - ntot) - 1;
          if (ind >= 0) os << records[j][ind] << "\t";
          else os << "      ---      " << "\t";
        }
        os << "\n";
      }
    }
    os << "recent ev analysis:\n";
    Ndim = (int)records.size();
    for (int j = 0; j < Ndim - 1; j++) {
      const int Nvar = 2 * (Ndim - j) + 1, N = (int)records[j].size();
      if (N < Nvar) continue;
      double sum1 = 0, sum2 = 0;
      for (int i = N - Nvar; i < N; i++) {
        const double ev = records[j][i];
        volatile double sq = ev * ev;
        sum1 += ev;
        sum2 += sq;
      }
      const double mean = sum1 / Nvar;
      volatile double sm = sum1 * mean;
      const double variance = (sum2 - sm) / (Nvar - 1);
      const double stderr_ = std::sqrt(variance / Nvar);
      os << j << ": N=" << Nvar << " <ev>=" << sum1 / Nvar << " sigma=" << std::sqrt(variance) << " StdErr=" << stderr_ << "\n";
      if (stderr_ < best_stderr) best_stderr = stderr_;
    }
    return os.str();
  }
  // checkpoint: the records, evidence_count, the best stderr
  void write(std::ostream& os) const {
    const int32_t head[3] = {evidence_count, records_dim, (int32_t)records.size()};
    os.write((const char*)head, sizeof head);
    os.write((const char*)&best_stderr, 8);
    for (size_t j = 0; j < records.size(); j++) {
      const uint64_t n = records[j].size();
      os.write((const char*)&n, 8);
      os.write((const char*)records[j].data(), (std::streamsize)(n * 8));
    }
  }
  bool read(std::istream& is) {
    int32_t head[3];
    double best = 0;
    is.read((char*)head, sizeof head);
    is.read((char*)&best, 8);
    if (!is || head[0] < 0 || head[2] < 0 || head[2] > 31 || head[1] != head[2]) return false;
    std::vector<std::vector<double> > rec((size_t)head[2]);
    for (size_t j = 0; j < rec.size(); j++) {
      uint64_t n = 0;
      is.read((char*)&n, 8);
      if (!is || n > (uint64_t)head[0]) return false;
      rec[j].resize((size_t)n);
      is.read((char*)rec[j].data(), (std::streamsize)(n * 8));
      if (!is) return false;
    }
    records.swap(rec); evidence_count = head[0]; records_dim = head[1]; best_stderr = best;
    return true;
  }
};

// A small persistent worker pool for the likelihood batches: starting and joining threads for every batch costs more than
// a cheap plug-in's whole batch.  run(n, chunk, f) calls f(k0, k1) over [0, n) in chunks, on the workers and the caller.
class eval_pool {
  // Workers sleep on a condition variable between batches.  PTM_EVAL_SPIN_US=<us> lets them SPIN that long for the next batch first (a
  // running sampler hands one over every ~50-100 us; a sleeping thread takes ~50 us to wake, the whole batch of a 128-chain ladder) --
  // an OpenMP runtime's active wait policy.  Not the default: on a shared host it is a gamble (the LISA example at 128 temperatures,
  // spinning / one thread, on two boxes of the pool: 76 / 102 and 117 / 84 us per step), and spinning workers eat a container's CPU quota.
  std::vector<std::thread> workers;
  std::mutex m;
  std::condition_variable cv_go, cv_done;
  std::function<void(int, int)> job;
  std::atomic<int> next{0}, gen{0}, busy{0}, sleepers{0};
  std::atomic<bool> stop{false};
  int n = 0, chunk = 1;
  long long spin_ns = 0;
  static long long now_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  static void relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
  }
  void drain() {
    for (;;) {
      const int k0 = next.fetch_add(chunk);
      if (k0 >= n) return;
      job(k0, k0 + chunk < n ? k0 + chunk : n);
    }
  }
  void loop(int seen) {   // `seen`: the generation current when this worker was created (resize() holds the mutex)
    for (;;) {
      bool got = false;
      for (const long long t0 = now_ns(); spin_ns > 0 && now_ns() - t0 < spin_ns;) {
        if (stop.load(std::memory_order_acquire)) return;
        if (gen.load(std::memory_order_acquire) != seen) { got = true; break; }
        for (int k = 0; k < 32; k++) relax();
      }
      if (!got) {
        std::unique_lock<std::mutex> lk(m);
        sleepers.fetch_add(1);
        cv_go.wait(lk, [&] { return stop.load() || gen.load() != seen; });
        sleepers.fetch_sub(1);
        if (stop.load()) return;
      }
      seen = gen.load(std::memory_order_acquire);
      drain();
      if (busy.fetch_sub(1, std::memory_order_acq_rel) == 1) { std::lock_guard<std::mutex> lk(m); cv_done.notify_one(); }
    }
  }

 public:
  eval_pool() { if (const char* v = getenv("PTM_EVAL_SPIN_US")) spin_ns = (long long)(atof(v) * 1e3); }
  ~eval_pool() {
    { std::lock_guard<std::mutex> lk(m); stop.store(true); }
    cv_go.notify_all();
    for (auto& t : workers) t.join();
  }
  int size() const { return (int)workers.size(); }
  void resize(int nworkers) {
    std::lock_guard<std::mutex> lk(m);   // a new worker starts from the current generation: it waits for the NEXT run
    while ((int)workers.size() < nworkers) {
      const int g = gen.load();
      workers.emplace_back([this, g] { loop(g); });
    }
  }
  void run(int n_, int chunk_, const std::function<void(int, int)>& f) {
    // (every worker has left the batch before: run() returns only when `busy` is back to zero)
    job = f; n = n_; chunk = chunk_ < 1 ? 1 : chunk_;
    next.store(0); busy.store((int)workers.size());
    gen.fetch_add(1);   // (sequentially consistent, like the workers' `sleepers` count: one of the two sides always sees the other's write)
    if (sleepers.load() > 0) { std::lock_guard<std::mutex> lk(m); cv_go.notify_all(); }   // (a worker on its way to sleep checks `gen` under the mutex)
    drain();
    for (const long long t0 = now_ns(); busy.load(std::memory_order_acquire) != 0;) {
      if (now_ns() - t0 > 2000000) {   // a worker that sleeps or was descheduled: wait for it without burning this thread
        std::unique_lock<std::mutex> lk(m);
        cv_done.wait(lk, [&] { return busy.load() == 0; });
        break;
      }
      relax();
    }
  }
};

// ---- bayesian.hh: the likelihood plug-in -----------------------------------------------------------------------------
class bayes_likelihood : public probability_function, public Optioned {  // bayesian.hh:307-581 (minimal interface)
 protected:
  stateSpace nativeSpace;
  std::shared_ptr<const sampleable_probability_function> nativePrior;
  double (*user_evaluate_log)(void* object, const state& s);
  void* user_object;
  bool evaluate_log_registered;
  double best_post;
  std::atomic<double> best_seen;   // best_post as the evaluating threads may read it without the mutex (it only ever grows)
  state best;
  std::mutex best_mutex;
  std::vector<double> likelyScales;
  bool have_scales;
  std::vector<proposal_distribution*> proposals;   // likelihood-associated proposals (bayesian.hh:784-790), owned
  std::vector<double> prop_shares;

 public:
  bool check_posterior;
  bayes_likelihood() : probability_function(nullptr), user_evaluate_log(nullptr), user_object(nullptr),
                       evaluate_log_registered(false), best_post(-INFINITY), best_seen(-INFINITY), have_scales(false), check_posterior(true) {}
  ~bayes_likelihood() { for (auto p : proposals) delete p; }
  bayes_likelihood(const bayes_likelihood&) = delete;
  void addOptions(Options& opt, const std::string& prefix = "") override { Optioned::addOptions(opt, prefix); }
  virtual void setup() {}   // the minimal interface has nothing to set up after basic_setup (bayesian.hh:394-405 is for data + signal)
  virtual void reset() {    // bayesian.hh:407-412
    best_post = -INFINITY;
    best_seen.store(-INFINITY);
    if (space) best = state(space, space->size()).scalar_mult(0);
  }
  virtual state bestState() { return best; }
  virtual double bestPost() { return best_post; }
  virtual void getScales(std::vector<double>& scales) {   // bayesian.hh:384-391
    if (have_scales) scales = likelyScales;
    else getObjectPrior()->getScales(scales);
  }
  void addProposal(const proposal_distribution* proposal, double share = 1) { proposals.push_back(proposal->clone()); prop_shares.push_back(share); }
  std::vector<proposal_distribution*> get_proposals() const { return proposals; }
  std::vector<double> get_prop_shares() const { return prop_shares; }
  void basic_setup(const stateSpace* sp, sampleable_probability_function* prior) {  // bayesian.hh:345-358
    nativeSpace = *sp;
    nativePrior.reset(prior);
    space = &nativeSpace;
    best = state(space, space->size());
    reset();
  }
  void basic_setup(const stateSpace* sp, const std::vector<std::string>& types, const std::vector<double>& centers,
                   const std::vector<double>& priorScales) {  // bayesian.hh:360-381
    std::valarray<int> t(types.size());
    for (size_t i = 0; i < types.size(); i++) {
      const std::string& s = types[i];
      if (s == "uni" || s == "uniform") t[i] = mixed_dist_product::uniform;
      else if (s == "gauss" || s == "gaussian") t[i] = mixed_dist_product::gaussian;
      else if (s == "pol" || s == "polar") t[i] = mixed_dist_product::polar;
      else if (s == "cpol" || s == "copol") t[i] = mixed_dist_product::copolar;
      else if (s == "log") t[i] = mixed_dist_product::log;
      else { std::cout << "bayes_likelihood::basic_setup: unknown prior type '" << s << "'" << std::endl; exit(1); }
    }
    nativeSpace = *sp;
    basic_setup(sp, new mixed_dist_product(&nativeSpace, t, std::valarray<double>(centers.data(), centers.size()),
                                           std::valarray<double>(priorScales.data(), priorScales.size())));
  }
  void register_reference_object(void* object) { user_object = object; }
  void register_evaluate_log(double (*function)(void* object, const state& s)) {
    user_evaluate_log = function;
    evaluate_log_registered = true;
  }
  std::shared_ptr<const sampleable_probability_function> getObjectPrior() const {
    if (!nativePrior) { std::cout << "bayes_component::getObjectPrior: No prior is defined for this object!" << std::endl; exit(1); }
    return nativePrior;
  }
  const stateSpace* getObjectStateSpace() const { return &nativeSpace; }
  // host evaluation of the plug-in (bayesian.hh:553-581), with the reference's best-posterior bookkeeping (quirk Q8: the
  // prior is evaluated again here, on the host, and the best log-posterior seen so far and its state are kept under a lock;
  // a posterior that is not finite turns the likelihood into -inf -- the reference also prints a warning for every such
  // state, this build only for NaN / +inf: a -inf likelihood outside the support is ordinary)
  double evaluate_log(state& s) override {
    if (!evaluate_log_registered) { std::cout << "bayes_component::panic!\nNo evaluate_log function is registered" << std::endl; exit(1); }
    double result = (*user_evaluate_log)(user_object, s);
    if (check_posterior) {
      const double lprior = nativePrior ? nativePrior->evaluate_log(s) : 0.0;
      const double post = result + lprior;
      // (the mutex only for a state that may be a new best: sixteen threads taking it for every evaluation evaluate one after the other)
      if (!(post <= best_seen.load(std::memory_order_relaxed))) {
        std::lock_guard<std::mutex> lk(best_mutex);
        if (!(post <= best_post)) { best_post = post; best = s; best_seen.store(post, std::memory_order_relaxed); }   // (a NaN sticks, as in the unguarded form)
      }
      if (!std::isfinite(post)) {
        if (!(post < 0)) std::cout << "Logpost is NAN!\n  params=" << s.get_string() << "\n  like=" << result << "  post=" << post << std::endl;
        result = -INFINITY;
      }
    }
    return result;
  }
  // device-resident targets override this and return true after describing themselves to the engine
  virtual bool describe_device_target(ptm_engine* e) { return false; }
  // C-ABI trampoline: the engine hands over the gated proposals of one sweep
  // The batch is spread over host threads -- the reference evaluates the rungs of one step under `omp parallel for`
  // (chain.cc:1544-1557) and so requires a thread-safe evaluate_log already; set_eval_threads(1) serialises.
  void set_eval_threads(int n) { eval_threads = n; }
  static void batch_trampoline(void* self, const double* X, int n, int dim, double* out) {
    bayes_likelihood* l = (bayes_likelihood*)self;
    auto work = [l, X, dim, out](int k0, int k1) {
      for (int k = k0; k < k1; k++) {
        state s = state::from_engine(l->getObjectStateSpace(), X + (size_t)k * dim, dim);   // (enforced on the device already)
        out[k] = l->evaluate_log(s);
      }
    };
    // (half of the usable processors: this thread and the HIP runtime's own need some, and a container's CPU quota throttles EVERY
    //  thread of the process once it is used up)
    int nt = l->eval_threads > 0 ? l->eval_threads : (usable_cpus() + 1) / 2;
    if (nt > n / 16) nt = n / 16;    // at least 16 states per thread
    // waking sleeping workers costs ~50 us: a batch that the measured cost per evaluation prices below ~4 such units stays on this
    // thread -- 30 us if the workers spin for their batches (PTM_EVAL_SPIN_US) (eval_threads == 0 only; an explicit thread count is obeyed)
    static const double pool_from_ns = [] {
      const char* v = getenv("PTM_EVAL_POOL_NS");
      if (v && *v) return atof(v);
      const char* sp = getenv("PTM_EVAL_SPIN_US");
      return (sp && atof(sp) > 0) ? 30e3 : 200e3;
    }();
    if (l->eval_threads <= 0 && l->eval_ns >= 0 && (l->eval_ns * n < pool_from_ns || l->pool_off)) nt = 1;
    if (nt <= 1) {
      const auto t0 = std::chrono::steady_clock::now();
      work(0, n);
      const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
      if (n > 0) l->eval_ns = l->eval_ns < 0 ? ns / n : 0.8 * l->eval_ns + 0.2 * ns / n;
      return;
    }
    if (!l->pool) l->pool.reset(new eval_pool);
    l->pool->resize(nt - 1);   // the calling thread works too
    const auto t0 = std::chrono::steady_clock::now();
    l->pool->run(n, (n + 4 * nt - 1) / (4 * nt), work);
    // does the pool pay on this machine?  (a container may show more hardware threads than it lets the process use; a likelihood may
    // serialise itself.)  Three batches in a row that cost more per evaluation than 0.7 of this thread alone: no pool from then on.
    if (l->eval_threads <= 0 && l->eval_ns > 0 && n > 0) {
      const double per = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / n;
      if (per > 0.7 * l->eval_ns) { if (++l->pool_bad >= 3) l->pool_off = true; }
      else l->pool_bad = 0;
    }
  }
  // the processors this process may really use: hardware threads, cut by its affinity mask and by a cgroup CPU quota
  // (PTM_EVAL_THREADS overrides)
  static int usable_cpus() {
    static const int n = [] {
      int c = (int)std::thread::hardware_concurrency();
      if (c < 1) c = 1;
#ifdef __linux__
      cpu_set_t set;
      if (sched_getaffinity(0, sizeof set, &set) == 0) { const int k = CPU_COUNT(&set); if (k > 0 && k < c) c = k; }
      {
        std::ifstream f2("/sys/fs/cgroup/cpu.max");   // cgroup v2: "<quota|max> <period>"
        std::string q;
        long long per = 0;
        if (f2 >> q >> per && q != "max" && per > 0) { const long long k = (atoll(q.c_str()) + per - 1) / per; if (k >= 1 && k < c) c = (int)k; }
        std::ifstream fq("/sys/fs/cgroup/cpu/cpu.cfs_quota_us"), fp("/sys/fs/cgroup/cpu/cpu.cfs_period_us");   // cgroup v1
        long long q1 = 0, p1 = 0;
        if (fq >> q1 && fp >> p1 && q1 > 0 && p1 > 0) { const long long k = (q1 + p1 - 1) / p1; if (k >= 1 && k < c) c = (int)k; }
      }
#endif
      if (const char* v = getenv("PTM_EVAL_THREADS")) { const int k = atoi(v); if (k >= 1) c = k; }
      return c;
    }();
    return n;
  }

 private:
  int eval_threads = 0;   // 0: all hardware threads
  double eval_ns = 0;     // running estimate of one evaluation's cost (the first batch runs serially and measures it)
  int pool_bad = 0;       // batches in a row that the pool made no faster
  bool pool_off = false;  // ... three of them: this likelihood stays on the calling thread
  std::unique_ptr<eval_pool> pool;

 public:
};

// A likelihood evaluated ON THE DEVICE (ptm_set_target_device): the engine calls evaluate_log_device once per sweep on its own stream
// with the batch of proposals in device memory (X_dev [n_rows][dim], rows [0, *count_dev) to evaluate, the rest in-support states);
// it enqueues its work on `stream` (a hipStream_t) and returns.  The host evaluate_log (register_evaluate_log) stays required: with a
// prior that is not a per-dimension product or with host-side proposals the ladder keeps the host path, and PTM_DEVICE_LIKE=0 in the
// environment forces it.  bestPost / bestState: the best of what the host path saw and of every engine this likelihood served on the
// device (replicas, walker ranges; ptm_get_best_evaluated -- an engine's is kept when the engine goes).
class device_likelihood : public bayes_likelihood {
 protected:
  std::vector<ptm_engine*> dev_engines;   // live engines that evaluate through this likelihood
  double dev_best_post = -INFINITY;       // the best of the engines already gone, and its state
  std::vector<double> dev_best_x;
  std::mutex dev_mutex;

 public:
  ~device_likelihood() {
    std::lock_guard<std::mutex> lk(engine_hooks_mutex());
    for (ptm_engine* e : dev_engines) engine_release_hooks().erase(e);
  }
  virtual void evaluate_log_device(void* stream, int n_rows, int dim, const double* X_dev, const int32_t* count_dev, double* out_dev) = 0;
  static void device_trampoline(void* self, void* stream, int n_rows, int dim, const double* X_dev, const int32_t* count_dev, double* out_dev) {
    ((device_likelihood*)self)->evaluate_log_device(stream, n_rows, dim, X_dev, count_dev, out_dev);
  }
  bool describe_device_target(ptm_engine* e) override {
    const char* v = getenv("PTM_DEVICE_LIKE");
    if (v && *v == '0') return false;
    ptm_check(ptm_set_target_device(e, &device_likelihood::device_trampoline, this, nullptr, nullptr), "set_target_device");
    {
      std::lock_guard<std::mutex> lk(dev_mutex);
      dev_engines.push_back(e);
    }
    std::lock_guard<std::mutex> lk(engine_hooks_mutex());
    engine_release_hooks()[e] = [this](ptm_engine* g) { release(g); };
    return true;
  }
  double bestPost() override {
    std::vector<double> x;
    return best_of_devices(x);
  }
  state bestState() override {
    std::vector<double> x;
    best_of_devices(x);
    return x.empty() ? best : state::from_engine(getObjectStateSpace(), x.data(), (int)x.size());
  }

 private:
  // an engine about to be destroyed: keep its best
  void release(ptm_engine* e) {
    std::vector<double> xe((size_t)nativeSpace.size() + 1);
    double lp = -INFINITY;
    const bool ok = ptm_get_best_evaluated(e, &lp, xe.data()) == PTM_OK;
    std::lock_guard<std::mutex> lk(dev_mutex);
    if (ok && lp > dev_best_post) { dev_best_post = lp; dev_best_x.assign(xe.begin(), xe.begin() + nativeSpace.size()); }
    dev_engines.erase(std::remove(dev_engines.begin(), dev_engines.end(), e), dev_engines.end());
  }
  // the host path's best, replaced by a strictly greater one of the engines (x: that state; empty if the host's stands)
  double best_of_devices(std::vector<double>& x) {
    double b = best_post;
    x.clear();
    std::lock_guard<std::mutex> lk(dev_mutex);
    if (dev_best_post > b) { b = dev_best_post; x = dev_best_x; }
    const int D = (int)nativeSpace.size();
    std::vector<double> xe(D > 0 ? D : 1);
    for (ptm_engine* e : dev_engines) {
      double lp = -INFINITY;
      if (ptm_get_best_evaluated(e, &lp, xe.data()) != PTM_OK) continue;
      if (lp > b) { b = lp; x.assign(xe.begin(), xe.begin() + D); }
    }
    return b;
  }
};

// correlated Gaussian target evaluated ON the device: like0 - 1/2 (x-mean)^T P (x-mean) (cython/exampleGaussian.py:46-109)
class gaussian_likelihood : public bayes_likelihood {
  std::vector<double> mean, precision;
  double like0;

 public:
  gaussian_likelihood(const std::vector<double>& precision_row_major, double like0, const std::vector<double>& mean = std::vector<double>())
      : mean(mean), precision(precision_row_major), like0(like0) {}
  bool describe_device_target(ptm_engine* e) override {
    ptm_check(ptm_set_target_gaussian(e, mean.empty() ? nullptr : mean.data(), precision.data(), like0), "gaussian_likelihood");
    return true;
  }
  double evaluate_log(state& s) override {
    const int D = s.size();
    double q = 0;
    for (int i = 0; i < D; i++)
      for (int j = 0; j < D; j++)
        q += (s.get_param(i) - (mean.empty() ? 0 : mean[i])) * precision[i * D + j] * (s.get_param(j) - (mean.empty() ? 0 : mean[j]));
    return like0 - 0.5 * q;
  }
};

class parallel_tempering_chains : public chain {  // chain.hh:214-330, chain.cc:1163-1571
  const int Ntemps, add_every_N;
  const double Tmax, swap_rate, dpriormin;
  ptm_engine* eng;
  const stateSpace* sp;
  int dim, nstep, hist_rows, hist_rungs = 0;   // hist_rungs: the coldest rungs whose saved states are kept (0: all)
  int Woff = 0, eng_device = -1;   // first GLOBAL replica of this engine, its device (set_replica_range)
  int W;   // independent replicas of the ladder run side by side (the reference runs its Nchain repeats one after the
           // other, ptmcmc.cc main loop): chain (rung i, replica w) sits at index i*W + w of every engine array
  std::vector<double> temps, X, llike, lpost;
  bool fresh, hist_fresh = false;
  size_t hist_have = 0;       // history chains [0, hist_have) are in hx / hl / hp / hmeta / hb (when hist_fresh)
  int hist_read_rungs = 0;    // > 0: a read-back fetches this many rungs (limit_history_reads), 0: all that keep history
  // replica-exchange diagnostics of chain.cc:1346-1356,1448-1451,1495-1498 (directions / instances / ups / downs), kept
  // on the host by replaying each step's candidate log (replica 0); on after track_exchanges(true)
  bool tracking = false;
  std::vector<int> directions, instances;
  std::vector<long> ups, downs;
  std::vector<int32_t> log_pairs, log_acc;
  void fetch_swaps() {
    const int ms = ptm_max_swaps_per_step(eng);
    log_pairs.resize((size_t)W * ms); log_acc.resize((size_t)W * ms);
    ptm_check(ptm_get_last_swaps(eng, log_pairs.data(), log_acc.data()), "replay_step");
  }
  void replay_swaps() {   // the loop of chain.cc:1436-1537, bookkeeping part, in pick order
    const int ms = ptm_max_swaps_per_step(eng);
    for (int j = 0; j < ms; j++) {
      const int i = log_pairs[j];
      if (i < 0) continue;
      if (i > 0) {                                   // chain.cc:1448-1451
        if (directions[i] > 0) ups[i]++;
        if (directions[i] < 0) downs[i]++;
      }
      if (log_acc[j]) {                              // chain.cc:1495-1498
        std::swap(directions[i], directions[i + 1]);
        std::swap(instances[i], instances[i + 1]);
        if (i == 0) directions[i] = 1;
        if (i + 1 == Ntemps - 1) directions[i + 1] = -1;
      }
    }
  }
  std::vector<double> hx, hl, hp;       // host copy of the history ring (dumpChain)
  std::vector<int32_t> hmeta;
  std::vector<int64_t> hnhist;
  std::vector<double> hb;
  std::vector<proposal_distribution*> props;

  // ---- host-side proposals (anything set_proposal cannot describe to the device as a fixed Gaussian) --------------------
  // The engine calls back once per sweep with the current states of every chain that moves (ptm_set_proposal_callback);
  // each chain's own clone of the proposal draws for it, with the chain's view as `caller`.  A host MIRROR of what
  // MH_chain::add_state saves (chain.cc:935-946) is kept for the proposals that read the chain history (differential
  // evolution): all Ninit initial draws, then every saved row, pulled from the device's short history ring after each step.
  bool host_mode = false, want_host = false;
  bool want_de = false, de_built = false;   // differential evolution drawn on the device from the device's history
  bool adaptive_dev = false;                // the proposal is an adaptive set drawn and adapted on the device (ptm_set_proposal_adaptive)
  bool prior_dev = false;                   // a member of the set draws from the prior on the device (ptm_set_proposal_prior_draw)
  bool user_dev = false;                    // the proposal is a device_proposal drawn on the device (ptm_set_proposal_device)
  int ring_rows = 0, ring_rungs = 0;   // the device history ring as the engine was created with it
  uint64_t eng_seed = 0;
  struct mirror_t {   // one chain's saved history, raw indexing as MH_chain::states / lposts / llikes (chain.hh:155-163)
    std::vector<double> x, llike, lprior, beta;
    std::vector<int32_t> meta;   // {Naccept, Ntries, type} per row
    size_t rows() const { return llike.size(); }
  };
  std::vector<mirror_t> mirror;        // [i*W + w]
  std::vector<int64_t> mirror_seen;    // device ring rows already copied (row numbers < this)
  int Ninit_rows = 1, Ninit_asked = 1;   // initial rows in the mirror / initial draws initialize() was asked for
  std::vector<std::vector<double> > init_x;            // the extra initial draws of initialize(n > 1): [k][chain*dim]
  std::vector<std::vector<double> > init_ll, init_lp;  // [k][chain]

  class rung_view : public chain {
    parallel_tempering_chains* p;
    int i, w;
    std::shared_ptr<philox_random> rng;

   public:
    rung_view(parallel_tempering_chains* p, int i, int w = 0) : p(p), i(i), w(w), rng(new philox_random) {}
    void step() override { std::cout << "rung_view::step: step the ladder, not a rung" << std::endl; exit(1); }
    size_t at() const { return (size_t)i * p->W + w; }
    // elem < 0 (or out of range): the current state; raw indexing: row `elem` of the saved history (host mirror, kept when
    // host-side proposals are in use); nominal indexing: step `elem` -> row Ninit + elem / add_every_N (chain.cc:1041-1050)
    bool hist_row(int elem, bool raw, size_t& row) {
      if (!p->host_mode || elem < 0) return false;
      const mirror_t& m = p->mirror[at()];
      const long r = raw ? elem : p->Ninit_rows + elem / p->add_every_N;
      if (r < 0 || (size_t)r >= m.rows()) return false;
      row = (size_t)r;
      return true;
    }
    state getState(int elem = -1, bool raw = false) override {
      size_t r;
      if (hist_row(elem, raw, r)) return state::from_engine(p->sp, p->mirror[at()].x.data() + r * p->dim, p->dim);
      p->refresh();
      return state::from_engine(p->sp, p->X.data() + at() * p->dim, p->dim);
    }
    double getLogPost(int elem = -1, bool raw = false) override {
      size_t r;
      if (hist_row(elem, raw, r)) { const mirror_t& m = p->mirror[at()]; const double t = m.beta[r] * m.llike[r]; return m.lprior[r] + t; }
      p->refresh();
      return p->lpost[at()];
    }
    double getLogLike(int elem = -1, bool raw = false) override {
      size_t r;
      if (hist_row(elem, raw, r)) return p->mirror[at()].llike[r];
      p->refresh();
      return p->llike[at()];
    }
    double invTemp() override { return p->cur_beta(i, w); }
    int getStep() override { return p->nstep; }
    int size() override { return p->host_mode ? (int)p->mirror[at()].rows() : p->nstep + 1; }
    int getDim() override { return p->dim; }
    int get_id() override { return (int)(w * p->Ntemps + i); }
    std::shared_ptr<Random> getPRNG() override { return rng; }
    void reseat(uint64_t seed, uint64_t step) { rng->reseat(seed, (uint32_t)((uint64_t)(w + p->Woff) * p->Ntemps + i), step); }
    double getMAPlpost() override { p->refresh_map(); return p->mlpost[at()]; }
    state getMAPstate() override { p->refresh_map(); return state::from_engine(p->sp, p->mX.data() + at() * p->dim, p->dim); }
  };
  std::vector<rung_view> views;
  // one replica's ladder as a chain: what a proposal that mixes the parallel chains' histories is given (chain.cc:1376-1378)
  class ladder_view : public chain {
    parallel_tempering_chains* p;
    int w;

   public:
    ladder_view(parallel_tempering_chains* p, int w) : p(p), w(w) {}
    void step() override { std::cout << "ladder_view::step: step the ladder itself" << std::endl; exit(1); }
    chain* cold() { return &p->views[(size_t)w * p->Ntemps]; }
    state getState(int elem = -1, bool raw = false) override { return cold()->getState(elem, raw); }
    double getLogPost(int elem = -1, bool raw = false) override { return cold()->getLogPost(elem, raw); }
    double getLogLike(int elem = -1, bool raw = false) override { return cold()->getLogLike(elem, raw); }
    int getStep() override { return p->nstep; }
    int size() override { return cold()->size(); }
    int getDim() override { return p->dim; }
    int multiplicity() override { return p->Ntemps; }
    chain* subchain(int index) override { return &p->views[(size_t)w * p->Ntemps + index]; }
    double getMAPlpost() override { return cold()->getMAPlpost(); }
    state getMAPstate() override { return cold()->getMAPstate(); }
  };
  std::vector<ladder_view> ladders;

  // the engine's callbacks (ptm_propose_batch_fn / ptm_proposal_result_fn)
  static void propose_trampoline(void* self, int n, int dim, const double* X_cur, const int32_t* rung, const int32_t* walker, uint64_t step,
                                 double* X_prop, double* log_hastings, int32_t* type, int32_t* valid) {
    parallel_tempering_chains* p = (parallel_tempering_chains*)self;
    p->fresh = false;   // (the temperatures an evolving ladder shows its proposals are this step's)
    for (int k = 0; k < n; k++) {
      const size_t v = (size_t)(walker[k] - p->Woff) * p->Ntemps + rung[k];   // (the engine names the GLOBAL walker)
      rung_view& view = p->views[v];
      view.reseat(p->eng_seed, step);
      state s = state::from_engine(p->sp, X_cur + (size_t)k * dim, dim);
      proposal_distribution* prop = p->props[v];
      state out = prop->draw(s, &view);
      for (int d = 0; d < dim; d++) X_prop[(size_t)k * dim + d] = out.get_param(d);
      log_hastings[k] = prop->log_hastings_ratio();
      type[k] = prop->type();
      valid[k] = out.invalid() ? 0 : 1;
    }
  }
  static void result_trampoline(void* self, int n, const int32_t* rung, const int32_t* walker, const int32_t* accepted) {
    parallel_tempering_chains* p = (parallel_tempering_chains*)self;
    for (int k = 0; k < n; k++) {
      proposal_distribution* prop = p->props[(size_t)(walker[k] - p->Woff) * p->Ntemps + rung[k]];
      if (accepted[k]) prop->accept(); else prop->reject();   // chain.cc:1009,1015
    }
  }
  // append what the last step(s) saved to the host mirror (rows the ring has not lost yet: call after every step)
  std::vector<double> rx, rl, rp, rb;
  std::vector<int32_t> rmeta;
  std::vector<int64_t> rnsize;
  void sync_history() { fetch_history(); append_history(); }
  void fetch_history() {
    const size_t HC = (size_t)Ntemps * W, cap = ring_rows;
    rx.resize(cap * HC * dim); rl.resize(cap * HC); rp.resize(cap * HC); rb.resize(cap * HC); rmeta.resize(cap * HC * 4); rnsize.resize(HC);
    ptm_check(ptm_get_array(eng, PTM_ARR_NSIZE, rnsize.data()), "sync_history");
    ptm_check(ptm_get_history(eng, rx.data(), rl.data(), rp.data(), rmeta.data()), "sync_history");
    ptm_check(ptm_get_history_invtemps(eng, rb.data()), "sync_history");
  }
  void append_history() {
    const size_t HC = (size_t)Ntemps * W, cap = ring_rows;
    for (size_t c = 0; c < HC; c++) {
      mirror_t& m = mirror[c];
      for (int64_t row = mirror_seen[c]; row < rnsize[c]; row++) {
        const size_t o = (size_t)(row % (int64_t)cap) * HC + c;
        if (rmeta[4 * o + 3] != (int32_t)row) { std::cout << "parallel_tempering_chains: the history ring lost rows before they were mirrored (step() n > ring / 2?)" << std::endl; exit(1); }
        m.x.insert(m.x.end(), rx.begin() + o * dim, rx.begin() + (o + 1) * dim);
        m.llike.push_back(rl[o]); m.lprior.push_back(rp[o]); m.beta.push_back(rb[o]);
        m.meta.push_back(rmeta[4 * o]); m.meta.push_back(rmeta[4 * o + 1]); m.meta.push_back(rmeta[4 * o + 2]);
      }
      mirror_seen[c] = rnsize[c];
    }
  }

  std::vector<double> mX, mlpost;   // host copy of the MAP states (chain.cc:931-934), all rungs / replicas
  bool map_fresh = false;
  void refresh_map() {
    if (map_fresh) return;
    mX.resize((size_t)Ntemps * W * dim); mlpost.resize((size_t)Ntemps * W);
    ptm_check(ptm_get_map(eng, mX.data(), mlpost.data(), nullptr, nullptr), "parallel_tempering_chains");
    map_fresh = true;
  }
  // evolve_temps (chain.hh:302-307): each replica's ladder owns its temperatures; betas [W][Ntemps] is their host copy
  double ev_rate = 0, ev_cut = -1;
  std::vector<double> betas;
  double cur_beta(int i, int w) {
    if (!(ev_rate > 0)) return 1 / temps[i];
    refresh();
    return betas[(size_t)w * Ntemps + i];
  }
  // ---- log-evidence by thermodynamic integration (chain.cc:1358-1360, 1577-1676): every istatsbin steps the total of every
  // replica's ladder over the last istatsbin add_state calls of its chains, from the device's own ring (ptm_log_evidence) or --
  // with host-side proposals, whose history is the host mirror, and with PTM_HOST_EVIDENCE=1 -- evidence_estimator here
  bool do_evid = false, verbose_evid = true;
  int istatsbin = 10000, icount = 0;
  std::vector<evidence_records> ev_records;            // [W]
  std::vector<double> ev_last, ev_up, ev_down;         // [W], [(Ntemps-1)*W] of the last epoch
  int evidence_rows() const { return istatsbin / add_every_N + 2; }
  static bool evidence_on_host() {
    static const bool on = [] { const char* v = getenv("PTM_HOST_EVIDENCE"); return v && *v && *v != '0'; }();   // (A/B: keep the host path)
    return on;
  }
  void evidence_epoch() {
    const size_t Wn = (size_t)W, np = (size_t)(Ntemps - 1) * Wn;
    ev_last.assign(Wn, 0.0); ev_up.assign(np, 0.0); ev_down.assign(np, 0.0);
    if (!host_mode && !evidence_on_host()) {
      ptm_check(ptm_log_evidence(eng, istatsbin, ev_last.data(), ev_up.data(), ev_down.data(), nullptr), "parallel_tempering_chains: log-evidence");
    } else {
      const size_t HC = (size_t)Ntemps * Wn, cap = (size_t)ring_rows;
      std::vector<int64_t> nh(HC);
      std::vector<double> rl;
      std::vector<int32_t> rm;
      ptm_check(ptm_get_array(eng, PTM_ARR_NHIST, nh.data()), "parallel_tempering_chains: log-evidence");
      if (!host_mode) {
        rl.resize(cap * HC); rm.resize(cap * HC * 4);
        ptm_check(ptm_get_history_chains(eng, 0, (int)HC, nullptr, rl.data(), nullptr, rm.data(), nullptr), "parallel_tempering_chains: log-evidence");
      }
      for (size_t w = 0; w < Wn; w++) {
        std::vector<long long> nhw((size_t)Ntemps);
        std::vector<double> bw((size_t)Ntemps);
        for (int i = 0; i < Ntemps; i++) { nhw[(size_t)i] = nh[(size_t)i * Wn + w]; bw[(size_t)i] = cur_beta(i, (int)w); }
        evidence_estimator::reader read;
        if (host_mode) read = [&, w](int rung, long long row, double& ll) {   // (the mirror counts its initial draws in front: chain.cc:1044)
          const mirror_t& m = mirror[(size_t)rung * Wn + w];
          const long long at = row - 1 + Ninit_rows;
          if (at < 0 || (size_t)at >= m.rows()) return false;
          ll = m.llike[(size_t)at];
          return true;
        };
        else read = [&, w](int rung, long long row, double& ll) {
          const size_t o = (size_t)(row % (long long)cap) * HC + (size_t)rung * Wn + w;
          if (rm[4 * o + 3] != (int32_t)row) return false;
          ll = rl[o];
          return true;
        };
        const evidence_estimator::result r = evidence_estimator::estimate(Ntemps, add_every_N, istatsbin, nhw.data(), bw.data(), read);
        if (!r.complete) { std::cout << "parallel_tempering_chains: the saved history no longer holds the evidence window (" << istatsbin << " steps)" << std::endl; exit(1); }
        ev_last[w] = r.evidence;
        for (int i = 0; i < Ntemps - 1; i++) { ev_up[(size_t)i * Wn + w] = r.up[(size_t)i]; ev_down[(size_t)i * Wn + w] = r.down[(size_t)i]; }
      }
    }
    // replica 0's lines are the reference's; with a population one more gives its spread
    for (size_t w = 0; w < Wn; w++) {
      const std::string lines = ev_records[w].push(ev_last[w], verbose_evid);
      if (w == 0) std::cout << lines << std::flush;
    }
    if (W > 1) {
      std::vector<double> e(ev_last);
      std::sort(e.begin(), e.end());
      std::cout << "Over " << e.size() << " replicas: log-evidence min=" << e.front() << " median=" << e[e.size() / 2] << " max=" << e.back() << std::endl;
    }
  }
  // the engine calls of n steps, cut where a statistics bin ends
  template <class F>
  void step_in_bins(int n, F advance) {
    while (n > 0) {
      const int k = do_evid ? std::min(n, std::max(1, istatsbin - icount)) : n;
      advance(k);
      n -= k;
      if (!do_evid) continue;
      icount += k;
      if (icount >= istatsbin) { evidence_epoch(); icount = 0; }   // chain.cc:1577, 1684
    }
  }
  void refresh() {
    if (fresh) return;
    ptm_check(ptm_batch_begin(eng), "parallel_tempering_chains");
    if (ev_rate > 0) {
      betas.resize((size_t)W * Ntemps);
      ptm_check(ptm_get_invtemps(eng, betas.data()), "parallel_tempering_chains");
    }
    ptm_check(ptm_get_states(eng, X.data()), "parallel_tempering_chains");
    ptm_check(ptm_get_array(eng, PTM_ARR_LLIKE, llike.data()), "parallel_tempering_chains");
    ptm_check(ptm_get_array(eng, PTM_ARR_LPOST, lpost.data()), "parallel_tempering_chains");
    ptm_check(ptm_batch_end(eng), "parallel_tempering_chains");
    fresh = true;
  }

 public:
  parallel_tempering_chains(int Ntemps, double Tmax, double swap_rate = 0.01, int add_every_N = 1, bool do_evid = false,
                            bool verbose_evid = true, double dpriormin = -30)
      : Ntemps(Ntemps), add_every_N(add_every_N), Tmax(Tmax), swap_rate(swap_rate), dpriormin(dpriormin), eng(nullptr),
        sp(nullptr), dim(0), nstep(0), hist_rows(0), W(1), temps(Ntemps, 1.0), fresh(false) {
    this->do_evid = do_evid && Ntemps > 1; this->verbose_evid = verbose_evid;
    istatsbin = 10000 * (add_every_N / 10 + 1);   // chain.cc:1358-1360
    // geometric ladder, chain.cc:1181-1183
    double tratio = Ntemps > 1 ? std::exp(std::log(Tmax) / (Ntemps - 1)) : 1.0;
    for (int i = 1; i < Ntemps; i++) temps[i] = temps[i - 1] * tratio;
  }
  ~parallel_tempering_chains() {
    if (eng) { engine_gone(eng); ptm_engine_destroy(eng); }
    for (auto p : props) delete p;
  }
  // Keep what MH_chain::add_state saves (every add_every_N-th state of every rung, chain.cc:935-946) on the device, in a
  // ring of `rows_per_chain` rows per rung; call before initialize().  The reference keeps the whole history in host
  // vectors; dumpChain() below writes the same file from the ring.
  // `coldest_rungs` > 0 keeps the history of that many rungs from the cold end only (what the sampler's pt_dump_n asks
  // for): less device memory, smaller read-backs.
  void keep_history(int rows_per_chain, int coldest_rungs = 0) {
    hist_rows = rows_per_chain;
    hist_rungs = coldest_rungs > 0 && coldest_rungs < Ntemps ? coldest_rungs : 0;
  }
  int history_rows() const { return hist_rows; }   // the slots of the history ring (ptm_get_history's capacity)
  int history_rungs() const { return hist_rows > 0 ? ((hist_rungs > 0 && !de_built) ? hist_rungs : Ntemps) : 0; }   // (differential evolution on the device: every rung's ring)
  // Run `n` independent replicas of the ladder in one engine (call before initialize()).  Replica w uses the random
  // streams of walker w; every accessor below takes the replica as an optional last argument (default 0).  Multiples
  // of 64 fill whole wavefronts and take the fast kernels.
  void set_replicas(int n) { W = n < 1 ? 1 : n; }
  // ---- the evidence (do_evid): the reference marks its bin of 10000 (add_every_N / 10 + 1) steps "make this user adjustable?";
  // set_stats_bin does (before initialize(): the history ring is sized by it).  bestEvidenceErr: the smallest standard error
  // of the recent totals so far (replica 0; 1e100 until six bins have passed), the sampler's pt_stop_evid_err criterion.
  void set_stats_bin(int steps) {
    if (steps < 1) steps = 1;
    if (eng && do_evid && steps > istatsbin) { std::cout << "parallel_tempering_chains::set_stats_bin: call before initialize() (the history ring holds " << istatsbin << " steps)" << std::endl; exit(1); }
    istatsbin = steps;
  }
  int stats_bin() const { return istatsbin; }
  bool evidence_on() const { return do_evid; }
  double bestEvidenceErr(int replica = 0) const { return do_evid && (size_t)replica < ev_records.size() ? ev_records[(size_t)replica].best() : 1e100; }
  int evidence_epochs() const { return ev_records.empty() ? 0 : ev_records[0].epochs(); }
  double lastEvidence(int replica = 0) const { return (size_t)replica < ev_last.size() ? ev_last[(size_t)replica] : 0.0 / 0.0; }
  const evidence_records& evidenceRecords(int replica = 0) const { return ev_records[(size_t)replica]; }
  // Several GPUs: one process per GPU, each with its own share of the replicas -- replicas `begin .. begin + n - 1` of the
  // population (call before initialize(); `device` < 0: the process's current device, e.g. through HIP_VISIBLE_DEVICES).
  // Replicas are independent ladders, so there is nothing to exchange between the processes, and a replica's chains are the
  // very ones a single engine holding the whole population gives it (ptm_config.walker_begin: its random streams are those of
  // the GLOBAL replica index) -- evolving ladders and host-side proposals included.
  void set_replica_range(int begin, int n, int device = -1) { Woff = begin < 0 ? 0 : begin; W = n < 1 ? 1 : n; eng_device = device; }
  int replica_begin() const { return Woff; }
  // Keep the reference's exchange diagnostics (which instance sits on which rung, round-trip directions, ups / downs)
  // for replica 0: costs one read-back of the step's candidate log per step, so it is off by default.
  void track_exchanges(bool on) {
    tracking = on;
    directions.assign(Ntemps, 0); instances.resize(Ntemps); ups.assign(Ntemps, 0); downs.assign(Ntemps, 0);
    for (int i = 0; i < Ntemps; i++) instances[i] = i;                       // chain.cc:1346-1356
    if (Ntemps > 0) { directions[0] = -1; directions[Ntemps - 1] = 1; }
    if (Ntemps == 1) directions[0] = -1;
  }
  // parallel_tempering_chains::evolve_temps (chain.hh:302-307): after every accepted exchange the gap between the two
  // temperatures is pried apart by (1 + rate) and the ladder renormalised (pry_temps, chain.cc:1501-1518,1809-1846).
  // Before or after initialize().  lpost_cut >= 0: the posterior-ordering cut (chain.cc:1819-1827).
  bool evolve_temps(double rate = 0.01, double lpost_cut = -1) {
    ev_rate = rate; ev_cut = lpost_cut;
    if (eng) { ptm_check(ptm_set_evolve_temps(eng, ev_rate, ev_cut), "evolve_temps"); fresh = false; }
    return true;
  }
  const std::vector<int>& getInstances() const { return instances; }
  const std::vector<int>& getDirections() const { return directions; }
  // parallel_tempering_chains::dumpTempStats (chain.cc:2025-2040): T, up fraction, swap acceptance of the pair above
  void dumpTempStats(std::ostream& os) {
    std::vector<int64_t> tries, acc;
    swap_counts(tries, acc);
    os << "#T0 up_frac0 up-swap_ratio0-1" << std::endl;
    for (int i = 0; i < Ntemps; i++) {
      double up_frac;
      if (i == 0) up_frac = 1;
      else if (i == Ntemps - 1) up_frac = 0;
      else up_frac = tracking ? ups[i] / (double)(ups[i] + downs[i]) : 0.0 / 0.0;
      os << 1 / cur_beta(i, 0) << " " << up_frac << " ";
      if (i < Ntemps - 1) os << acc[i] / (double)tries[i] << ": ";
      os << std::endl;
    }
    os << "\n" << std::endl;
  }
  int replicas() const { return W; }
  // chain::checkpoint / restart (chain.cc:1213-1290): everything the ladder's future depends on, into <path>chain0-cp/
  // PTchain.cp.  NOT interchangeable with the reference's checkpoint files: those hold its newran generators and growing
  // history vectors; this one holds the engine's arrays (states, llikes, MH_chain counters, step count = position of every
  // random stream, exchange counters, evolving temperatures, history ring, MAPs, the exchange diagnostics, and -- with
  // host-side proposals -- the host history mirror; the proposals checkpoint themselves beside it as in the reference) --
  // the continued run is the uninterrupted run, bit for bit.  The header names the format version and every parameter a
  // restart must share (sizes, seed, swap rate, add_every_N, ring shape, evolution, proposal placement); the whole file is
  // read and checked BEFORE anything is applied to the engine.
  struct cp_header {
    char magic[8];
    int32_t version, Ntemps, W, dim, add_every_N, ring_rows, ring_rungs, evolving, tracking, host_mode, Ninit_rows, nstep;
    uint64_t seed, engine_step;
    double swap_rate, Tmax;
  };
  void checkpoint(const std::string& path) {
    const std::string dir = path + "chain0-cp/";
    mkdir(dir.c_str(), 0777);
    std::ofstream os((dir + "PTchain.cp").c_str(), std::ios::binary);
    if (!os) { std::cout << "parallel_tempering_chains::checkpoint: cannot write " << dir << "PTchain.cp" << std::endl; exit(1); }
    const size_t N = (size_t)Ntemps * W, np = (size_t)W * (Ntemps > 1 ? Ntemps - 1 : 1);
    auto wr = [&](const void* ptr, size_t bytes) { os.write((const char*)ptr, (std::streamsize)bytes); };
    cp_header h;
    memset(&h, 0, sizeof h);
    memcpy(h.magic, "PTMGPU02", 8);
    h.version = 2; h.Ntemps = Ntemps; h.W = W; h.dim = dim; h.add_every_N = add_every_N; h.ring_rows = ring_rows; h.ring_rungs = ring_rungs;
    h.evolving = ev_rate > 0 ? 1 : 0; h.tracking = tracking ? 1 : 0; h.host_mode = host_mode ? 1 : 0; h.Ninit_rows = Ninit_rows; h.nstep = nstep;
    h.seed = eng_seed; h.engine_step = ptm_step_count(eng); h.swap_rate = swap_rate; h.Tmax = Tmax;
    wr(&h, sizeof h);
    std::vector<double> x(N * dim), ll(N);
    std::vector<int32_t> nt(N), na(N), ty(N);
    std::vector<int64_t> nh(N), st(np), sa(np);
    ptm_check(ptm_get_states(eng, x.data()), "checkpoint");
    ptm_check(ptm_get_array(eng, PTM_ARR_LLIKE, ll.data()), "checkpoint");
    ptm_check(ptm_get_array(eng, PTM_ARR_NTRIES, nt.data()), "checkpoint");
    ptm_check(ptm_get_array(eng, PTM_ARR_NACCEPT, na.data()), "checkpoint");
    ptm_check(ptm_get_array(eng, PTM_ARR_LAST_TYPE, ty.data()), "checkpoint");
    ptm_check(ptm_get_array(eng, PTM_ARR_NHIST, nh.data()), "checkpoint");
    ptm_check(ptm_get_swap_counts(eng, st.data(), sa.data()), "checkpoint");
    wr(x.data(), x.size() * 8); wr(ll.data(), N * 8); wr(nt.data(), N * 4); wr(na.data(), N * 4); wr(ty.data(), N * 4);
    wr(nh.data(), N * 8); wr(st.data(), np * 8); wr(sa.data(), np * 8);
    if (ev_rate > 0) {
      std::vector<double> b((size_t)W * Ntemps);
      ptm_check(ptm_get_invtemps(eng, b.data()), "checkpoint");
      wr(b.data(), b.size() * 8);
    }
    if (ring_rows > 0) {
      const size_t n = (size_t)ring_rows * ring_rungs * W;
      std::vector<double> gx(n * dim), gl(n), gp(n), gb(n);
      std::vector<int32_t> gm(n * 4);
      ptm_check(ptm_get_history(eng, gx.data(), gl.data(), gp.data(), gm.data()), "checkpoint");
      ptm_check(ptm_get_history_invtemps(eng, gb.data()), "checkpoint");
      wr(gx.data(), gx.size() * 8); wr(gl.data(), n * 8); wr(gp.data(), n * 8); wr(gm.data(), gm.size() * 4); wr(gb.data(), n * 8);
    }
    {
      std::vector<double> mx(N * dim), mp(N), ml(N), mr(N);
      ptm_check(ptm_get_map(eng, mx.data(), mp.data(), ml.data(), mr.data()), "checkpoint");
      wr(mx.data(), mx.size() * 8); wr(mp.data(), N * 8); wr(ml.data(), N * 8); wr(mr.data(), N * 8);
    }
    if (tracking) {
      std::vector<int64_t> u(ups.begin(), ups.end()), d(downs.begin(), downs.end());
      wr(directions.data(), (size_t)Ntemps * 4); wr(instances.data(), (size_t)Ntemps * 4); wr(u.data(), (size_t)Ntemps * 8); wr(d.data(), (size_t)Ntemps * 8);
    }
    if (host_mode) {
      for (size_t c = 0; c < N; c++) {
        const mirror_t& m = mirror[c];
        const uint64_t rows = m.rows();
        wr(&rows, 8); wr(&mirror_seen[c], 8);
        wr(m.x.data(), m.x.size() * 8); wr(m.llike.data(), rows * 8); wr(m.lprior.data(), rows * 8); wr(m.beta.data(), rows * 8); wr(m.meta.data(), m.meta.size() * 4);
      }
      for (auto pp : props) pp->checkpoint(dir);
    }
    if (!os) { std::cout << "parallel_tempering_chains::checkpoint: write failed" << std::endl; exit(1); }
    if (do_evid) {   // the evidence's own file: PTchain.cp holds the same bytes with and without it
      std::ofstream oe((dir + "PTevidence.cp").c_str(), std::ios::binary);
      const int32_t head[4] = {0x45564431, W, istatsbin, icount};
      oe.write((const char*)head, sizeof head);
      for (size_t w = 0; w < ev_records.size(); w++) ev_records[w].write(oe);
      if (!oe) { std::cout << "parallel_tempering_chains::checkpoint: cannot write " << dir << "PTevidence.cp" << std::endl; exit(1); }
    }
  }
  // into a ladder set up exactly like the one that was saved (same sizes, seed, likelihood, prior, proposal, evolve_temps)
  void restart(const std::string& path) {
    const std::string dir = path + "chain0-cp/", fn = dir + "PTchain.cp";
    std::ifstream is(fn.c_str(), std::ios::binary);
    if (!is) { std::cout << "parallel_tempering_chains::restart: cannot read " << fn << std::endl; exit(1); }
    std::vector<char> buf((std::istreambuf_iterator<char>(is)), std::istreambuf_iterator<char>());
    size_t pos = 0;
    bool ok = true;
    auto rd = [&](void* ptr, size_t bytes) { if (pos + bytes > buf.size()) { ok = false; return; } memcpy(ptr, buf.data() + pos, bytes); pos += bytes; };
    cp_header h;
    rd(&h, sizeof h);
    if (!ok || std::string(h.magic, 8) != "PTMGPU02" || h.version != 2) { std::cout << "parallel_tempering_chains::restart: " << fn << " is not a checkpoint of this build (format 2)" << std::endl; exit(1); }
    if (h.Ntemps != Ntemps || h.W != W || h.dim != dim || h.add_every_N != add_every_N || h.ring_rows != ring_rows || h.ring_rungs != ring_rungs ||
        h.evolving != (ev_rate > 0 ? 1 : 0) || h.host_mode != (host_mode ? 1 : 0) || h.seed != eng_seed || h.swap_rate != swap_rate || h.Tmax != Tmax) {
      std::cout << "parallel_tempering_chains::restart: " << fn << " was written by a differently configured ladder (sizes, seed, swap rate, Tmax, "
                << "history ring, evolution and proposal placement must all match)" << std::endl;
      exit(1);
    }
    const size_t N = (size_t)Ntemps * W, np = (size_t)W * (Ntemps > 1 ? Ntemps - 1 : 1);
    std::vector<double> x(N * dim), ll(N), b, gx, gl, gp, gb, mx(N * dim), mp(N), ml(N), mr(N);
    std::vector<int32_t> nt(N), na(N), ty(N), gm, dir_(Ntemps), ins_(Ntemps);
    std::vector<int64_t> nh(N), st(np), sa(np), u(Ntemps), d(Ntemps);
    rd(x.data(), x.size() * 8); rd(ll.data(), N * 8); rd(nt.data(), N * 4); rd(na.data(), N * 4); rd(ty.data(), N * 4);
    rd(nh.data(), N * 8); rd(st.data(), np * 8); rd(sa.data(), np * 8);
    if (ev_rate > 0) { b.resize((size_t)W * Ntemps); rd(b.data(), b.size() * 8); }
    const size_t nring = (size_t)ring_rows * ring_rungs * W;
    if (ring_rows > 0) {
      gx.resize(nring * dim); gl.resize(nring); gp.resize(nring); gb.resize(nring); gm.resize(nring * 4);
      rd(gx.data(), gx.size() * 8); rd(gl.data(), nring * 8); rd(gp.data(), nring * 8); rd(gm.data(), gm.size() * 4); rd(gb.data(), nring * 8);
    }
    rd(mx.data(), mx.size() * 8); rd(mp.data(), N * 8); rd(ml.data(), N * 8); rd(mr.data(), N * 8);
    if (h.tracking) { rd(dir_.data(), (size_t)Ntemps * 4); rd(ins_.data(), (size_t)Ntemps * 4); rd(u.data(), (size_t)Ntemps * 8); rd(d.data(), (size_t)Ntemps * 8); }
    std::vector<mirror_t> mir;
    std::vector<int64_t> seen;
    if (host_mode) {
      mir.resize(N); seen.resize(N);
      for (size_t c = 0; c < N && ok; c++) {
        uint64_t rows = 0;
        rd(&rows, 8); rd(&seen[c], 8);
        if (!ok || rows > buf.size()) { ok = false; break; }
        mirror_t& m = mir[c];
        m.x.resize(rows * dim); m.llike.resize(rows); m.lprior.resize(rows); m.beta.resize(rows); m.meta.resize(rows * 3);
        rd(m.x.data(), m.x.size() * 8); rd(m.llike.data(), rows * 8); rd(m.lprior.data(), rows * 8); rd(m.beta.data(), rows * 8); rd(m.meta.data(), m.meta.size() * 4);
      }
    }
    if (!ok || pos != buf.size()) { std::cout << "parallel_tempering_chains::restart: " << fn << " is truncated or has trailing bytes; nothing was applied" << std::endl; exit(1); }
    // ---- the file is whole and matches: apply
    ptm_check(ptm_restore(eng, x.data(), ll.data(), nt.data(), na.data(), ty.data(), nh.data(), h.engine_step, st.data(), sa.data()), "restart");
    if (ev_rate > 0) ptm_check(ptm_set_invtemps(eng, b.data()), "restart");
    if (ring_rows > 0) ptm_check(ptm_set_history(eng, gx.data(), gl.data(), gp.data(), gm.data(), gb.data()), "restart");
    ptm_check(ptm_set_map(eng, mx.data(), mp.data(), ml.data(), mr.data()), "restart");
    if (h.tracking) {
      track_exchanges(true);
      directions.assign(dir_.begin(), dir_.end()); instances.assign(ins_.begin(), ins_.end());
      ups.assign(u.begin(), u.end()); downs.assign(d.begin(), d.end());
    }
    if (host_mode) {
      mirror.swap(mir); mirror_seen.swap(seen); Ninit_rows = h.Ninit_rows;
      for (auto pp : props) pp->restart(dir);
    }
    nstep = h.nstep;
    fresh = hist_fresh = map_fresh = false;
    if (do_evid) {
      std::ifstream ie((dir + "PTevidence.cp").c_str(), std::ios::binary);
      int32_t head[4] = {0, 0, 0, 0};
      ie.read((char*)head, sizeof head);
      bool good = (bool)ie && head[0] == 0x45564431 && head[1] == W && head[2] == istatsbin && head[3] >= 0 && head[3] < istatsbin;
      std::vector<evidence_records> rec((size_t)W);
      for (size_t w = 0; good && w < rec.size(); w++) good = rec[w].read(ie);
      if (!good) { std::cout << "parallel_tempering_chains::restart: " << dir << "PTevidence.cp is missing or does not match this ladder (replicas, statistics bin)" << std::endl; exit(1); }
      ev_records.swap(rec);
      icount = head[3];
    }
  }
  // chain.cc:1281-1365: n prior draws per rung (the device draws them: any prior type but the improper flat one); the last one
  // is the chain's start, the others seed the history that history-reading proposals draw from (ptmcmc.cc:86: de_ni * Npar)
  bayes_likelihood* init_like = nullptr;
  const sampleable_probability_function* init_prior = nullptr;
  bool prior_on_host = false;   // the prior is not a per-dimension product: evaluated through ptm_set_prior_callback
  bool prior_on_device = false; // ... or, a device_prior beside a device_likelihood, through ptm_set_prior_device (start states still drawn on the host)
  // C-ABI trampoline of a host-evaluated prior: probability_function::evaluate_log on every (valid) state of the batch
  static void prior_trampoline(void* self, const double* X, int n, int dim, double* out) {
    const sampleable_probability_function* pr = (const sampleable_probability_function*)self;
    for (int k = 0; k < n; k++) {
      state s = state::from_engine(pr->get_space(), X + (size_t)k * dim, dim);   // (enforced on the device already)
      out[k] = pr->evaluate_log(s);
    }
  }
  std::vector<double> init_start;
  bool have_start = false;
  // tell the ladder BEFORE initialize() that its proposal will be drawn on the host (saves building the engine twice)
  void use_host_proposals(bool on = true) { want_host = on; }
  // ... or that its set holds a differential evolution the DEVICE draws (ptm_set_proposal_de): the engine then records every rung's
  // history (keep_history must hold the whole run) and keeps the n - 1 extra draws of initialize(n) on the device
  void use_device_de(bool on = true) { want_de = on; }
  bool draws_de_on_device() const { return de_built; }
  void initialize(bayes_likelihood* log_likelihood, const sampleable_probability_function* log_prior, int n = 1, uint64_t seed = 0x5EED0001ull,
                  const std::vector<double>* start_states = nullptr) {
    init_like = log_likelihood; init_prior = log_prior; Ninit_asked = n < 1 ? 1 : n; eng_seed = seed;
    have_start = start_states != nullptr;
    if (have_start) init_start = *start_states;
    build_engine(want_host);
  }

 private:
  // The device route of a prior that does not describe itself: a device_prior beside a device_likelihood that takes the device, proposals
  // not on the host, PTM_DEVICE_PRIOR not 0 in the environment.  Registers the likelihood (ptm_set_target_device) when it answers with
  // the prior; nullptr: today's host route, nothing registered.
  const device_prior* device_prior_route(bool host, bayes_likelihood* log_likelihood, const sampleable_probability_function* log_prior) {
    const device_prior* dpr = dynamic_cast<const device_prior*>(log_prior);
    if (!dpr || host || !device_prior::wanted()) return nullptr;
    if (!dynamic_cast<device_likelihood*>(log_likelihood)) return nullptr;
    return log_likelihood->describe_device_target(eng) ? dpr : nullptr;
  }
  void build_engine(bool host) {
    if (eng) { engine_gone(eng); ptm_engine_destroy(eng); eng = nullptr; }
    bayes_likelihood* log_likelihood = init_like;
    const sampleable_probability_function* log_prior = init_prior;
    sp = log_prior->get_space();
    dim = log_prior->getDim();
    host_mode = host;
    Ninit_rows = host ? Ninit_asked : 1;
    // differential evolution on the device: every rung's history stays there, in a ring as long as the run (keep_history), with the
    // extra draws of initialize(n) beside it; the rows keep the ring's numbering (row 0 = the start state)
    if (do_evid) {   // every rung's saved llikes of a whole statistics bin (with host-side proposals the host mirror has them)
      if (!host) {
        hist_rows = std::max(hist_rows, evidence_rows());
        hist_rungs = 0;
        const int dp = dim > 16 ? 32 * ((dim + 31) / 32) : (dim > 8 ? 16 : (dim > 4 ? 8 : 4));
        const double bytes = (double)hist_rows * Ntemps * W * (8.0 * dp + 40.0);
        if (bytes >= 16e9) {
          std::cout << "parallel_tempering_chains: the evidence needs " << hist_rows << " saved rows of all " << Ntemps << " rungs x " << W << " replicas on the device ("
                    << bytes / 1e9 << " GB, above the 16 GB limit): fewer replicas, a larger save_every or a shorter statistics bin" << std::endl;
          exit(1);
        }
      }
      ev_records.assign((size_t)W, evidence_records());
      icount = 0;
    }
    de_built = !host && want_de && hist_rows > 0;
    const int draws = (host || de_built) ? Ninit_asked : 1;
    // host-side proposals: every rung's saved rows pass through a SHORT device ring into the host mirror after each step
    ring_rows = host ? 8 : hist_rows;
    ring_rungs = (host || de_built) ? Ntemps : history_rungs();
    ptm_config cfg = ptm_config();   // (zeroed: fields a newer ABI adds default to 0)
    cfg.struct_size = sizeof cfg;
    cfg.dim = dim; cfg.n_rungs = Ntemps; cfg.rung_begin = 0; cfg.rung_count = Ntemps; cfg.n_walkers = W; cfg.seed = eng_seed;
    cfg.swap_rate = swap_rate; cfg.add_every_n = add_every_N; cfg.min_prior = dpriormin; cfg.device = eng_device; cfg.stream = nullptr;
    cfg.walker_begin = Woff;
    cfg.time_kernels = 0; cfg.swap_log_steps = 0; cfg.exchange_row_capacity = 0; cfg.history_rungs = ring_rungs; cfg.history_capacity = ring_rows; cfg.map_rungs = Ntemps;
    ptm_check(ptm_engine_create(&cfg, &eng), "parallel_tempering_chains::initialize");
    std::vector<int> lo(dim), hi(dim), types;
    std::vector<double> xmin(dim), xmax(dim), centers, halfwidths;
    for (int i = 0; i < dim; i++) {
      boundary b = sp ? sp->get_bound(i) : boundary();
      lo[i] = b.lower(); hi[i] = b.upper();
      b.getDomainLimits(xmin[i], xmax[i]);
      if (lo[i] == boundary::open && hi[i] == boundary::open) xmin[i] = xmax[i] = 0;
    }
    ptm_check(ptm_set_bounds(eng, lo.data(), hi.data(), xmin.data(), xmax.data()), "set_bounds");
    prior_on_host = !log_prior->describe(types, centers, halfwidths);
    prior_on_device = false;
    if (!prior_on_host) {
      ptm_check(ptm_set_prior(eng, types.data(), centers.data(), halfwidths.data()), "set_prior");
      // (a device likelihood cannot serve host-side proposals, whose step waits on the host anyway: its host evaluate_log does)
      const bool skip_device = host && dynamic_cast<device_likelihood*>(log_likelihood) != nullptr;
      if (skip_device || !log_likelihood->describe_device_target(eng))
        ptm_check(ptm_set_target_callback(eng, &bayes_likelihood::batch_trampoline, log_likelihood), "set_target_callback");
    } else if (const device_prior* dpr = device_prior_route(host, log_likelihood, log_prior)) {
      // ... but a device_prior beside a device_likelihood that took the device: both run on the engine's stream, the step stays there
      ptm_check(ptm_set_prior_device(eng, &device_prior::device_trampoline, (void*)dpr), "set_prior_device");
      prior_on_device = true;
    } else {
      // a prior that is not a per-dimension product: evaluated on the host between the propose and the accept kernel, and so
      // is the likelihood then (whatever it is: its evaluate_log)
      ptm_check(ptm_set_target_callback(eng, &bayes_likelihood::batch_trampoline, log_likelihood), "set_target_callback");
      ptm_check(ptm_set_prior_callback(eng, &parallel_tempering_chains::prior_trampoline, (void*)log_prior), "set_prior_callback");
    }
    std::vector<double> beta(Ntemps);
    for (int i = 0; i < Ntemps; i++) beta[i] = 1 / temps[i];  // chain.cc:1340
    ptm_check(ptm_set_ladder(eng, beta.data()), "set_ladder");
    if (ev_rate > 0) ptm_check(ptm_set_evolve_temps(eng, ev_rate, ev_cut), "evolve_temps");
    const size_t N = (size_t)Ntemps * W;
    X.assign(N * dim, 0.0); llike.assign(N, 0.0); lpost.assign(N, 0.0);
    init_x.clear(); init_ll.clear(); init_lp.clear();
    if (have_start) {
      ptm_check(ptm_set_states(eng, init_start.data(), nullptr), "set_states");
      Ninit_rows = 1;
    } else if (prior_on_host) {
      // MH_chain::initialize (chain.cc:846-876) on the host: every start state is a draw of the prior's own drawSample with the
      // chain's generator, redrawn while the likelihood is below -1e100 (:856-869); draws 1 .. n-1 are kept for the mirror
      std::vector<double> x0(N * dim);
      for (int k = draws - 1; k >= 0; k--) {
        std::vector<double> x(N * dim), ll(N), lp(N);
        for (size_t c = 0; c < N; c++) {
          philox_random rng;
          rng.reseat(eng_seed, (uint32_t)((c % W + Woff) * Ntemps + c / W), ((uint64_t)1 << 40) + (uint64_t)k);   // (a step no sweep reaches)
          for (int attempt = 0;; attempt++) {
            state s = log_prior->drawSample(rng);
            const double l = s.invalid() ? -INFINITY : log_likelihood->evaluate_log(s);
            if (!(l < -1e100)) {
              for (int d = 0; d < dim; d++) x[c * dim + d] = s.get_param(d);
              ll[c] = l; lp[c] = log_prior->evaluate_log(s);
              break;
            }
            if (attempt >= 100000) { std::cout << "parallel_tempering_chains::initialize: no valid start state drawn from the prior" << std::endl; exit(1); }
          }
        }
        if (k > 0) { init_x.push_back(x); init_ll.push_back(ll); init_lp.push_back(lp); }
        else x0 = x;
      }
      ptm_check(ptm_set_states(eng, x0.data(), nullptr), "set_states");
    } else {
      // draws 1 .. n-1 first (kept for the mirror; all of them in ONE call, the order of the rows as before: n-1 first), draw 0 last:
      // it is the chain's start, whatever n is
      if (draws > 1) {
        const size_t nd = (size_t)draws - 1;
        std::vector<double> ax(nd * N * dim), al(nd * N), ap(nd * N);
        int rc = ptm_draw_prior_rows(eng, 1, (int)nd, ax.data(), al.data(), ap.data());
        if (rc == PTM_ERR_UNSUPPORTED) {
          std::cout << "parallel_tempering_chains::initialize: " << ptm_last_error() << "; pass start states" << std::endl;
          exit(1);
        }
        ptm_check(rc, "draw_prior_rows");
        for (size_t k = nd; k >= 1; k--) {
          const size_t o = k - 1;   // (row of draw k)
          init_x.push_back(std::vector<double>(ax.begin() + o * N * dim, ax.begin() + (o + 1) * N * dim));
          init_ll.push_back(std::vector<double>(al.begin() + o * N, al.begin() + (o + 1) * N));
          init_lp.push_back(std::vector<double>(ap.begin() + o * N, ap.begin() + (o + 1) * N));
        }
      }
      int rc = ptm_init_from_prior_k(eng, 0);
      if (rc == PTM_ERR_UNSUPPORTED) {
        std::cout << "parallel_tempering_chains::initialize: " << ptm_last_error() << "; pass start states" << std::endl;
        exit(1);
      }
      ptm_check(rc, "init_from_prior");
    }
    views.clear(); ladders.clear();
    for (int w = 0; w < W; w++) {
      for (int i = 0; i < Ntemps; i++) views.push_back(rung_view(this, i, w));   // views[w*Ntemps + i]
      ladders.push_back(ladder_view(this, w));
    }
    fresh = hist_fresh = map_fresh = false;
    if (host) {
      // the mirror starts with the initial draws (MH_chain::initialize adds every one of them, chain.cc:846-876)
      mirror.assign(N, mirror_t());
      mirror_seen.assign(N, 0);
      for (size_t c = 0; c < N; c++) {
        const int i = (int)(c / W);
        for (size_t k = 0; k < init_x.size(); k++) {
          mirror_t& m = mirror[c];
          m.x.insert(m.x.end(), init_x[k].begin() + c * dim, init_x[k].begin() + (c + 1) * dim);
          m.llike.push_back(init_ll[k][c]); m.lprior.push_back(init_lp[k][c]); m.beta.push_back(beta[i]);
          m.meta.push_back(1); m.meta.push_back(1); m.meta.push_back(-1);
        }
      }
      sync_history();   // row 0 of the ring: the start state
    }
  }

 public:
  // chain.cc:1367-1386: one clone per rung (and replica); a proposal that supports mixing is given the whole ladder as its
  // chain, any other its own rung (set_chain).  Gaussians with a fixed factor -- and sets of scalar multiples of one -- are
  // drawn on the device; everything else through the host-proposal step.
  void set_proposal(proposal_distribution& proposal) {
    for (auto p : props) delete p;
    props.clear();
    user_dev = false;
    if (device_proposal::taken_by_device(&proposal)) {
      // a device_proposal: its draw_device runs on the engine's stream, the likelihood stays where it is (a device_likelihood: the whole
      // step on the device).  Every rung gets a clone (reports); the first serves the batch.
      if (host_mode) build_engine(false);
      for (int i = 0; i < Ntemps; i++) props.push_back(proposal.clone());
      device_proposal* dp = dynamic_cast<device_proposal*>(props[0]);
      ptm_check(ptm_set_proposal_device(eng, &device_proposal::device_trampoline, dp->has_result_device() ? &device_proposal::device_result_trampoline : nullptr, dp),
                "set_proposal_device");
      user_dev = true; adaptive_dev = false; prior_dev = false;
      return;
    }
    int kind = 0;
    double odf = 0;
    std::vector<double> f, all, odfs(Ntemps);
    bool on_device = true;
    for (int i = 0; i < Ntemps && on_device; i++) {
      const user_gaussian_prop* ug = dynamic_cast<const user_gaussian_prop*>(&proposal);
      if (!(ug ? ug->device_describe_in(sp, dim, kind, f, odf) : proposal.device_describe(dim, kind, f, odf))) { on_device = false; break; }
      all.insert(all.end(), f.begin(), f.end());
      odfs[i] = odf;
    }
    if (on_device && !prior_draws_fit_device(proposal, init_prior, prior_on_host)) on_device = false;
    {
      ptm_de_params q;
      if (on_device && proposal.device_describe_de(q)) {
        // a set with a differential evolution for the device: possible if the ring holds the run and the dimensions fit the kernel
        // that draws it (ptm_set_proposal_de); else the whole set is drawn on the host
        if (hist_rows <= 0 || dim > 32) on_device = false;
        else if (!de_built) { want_de = true; build_engine(false); }   // (initialize() did not know: set up again, with the same draws)
      }
    }
    if (on_device) {
      if (host_mode) build_engine(false);
      for (int i = 0; i < Ntemps; i++) props.push_back(proposal.clone());
      ptm_check(ptm_set_proposals(eng, kind, all.data(), odfs.data()), "set_proposals");
      dev_prop_kind = kind;
      std::vector<double> cum, sc, od;
      proposal_distribution_set* ps = dynamic_cast<proposal_distribution_set*>(&proposal);
      // temperature-dependent shares: every rung's clone builds its thresholds from the rung's temperature as it is now (set_chain,
      // proposal_distribution.hh:336) and hands them over below; nothing rebuilds them later (the top shares do not adapt)
      if (ps && ps->thermal())
        for (int i = 0; i < Ntemps; i++) props[i]->set_chain(&views[i]);
      ptm_adaptive_set as;
      int kind_a;
      std::vector<double> f_a;
      adaptive_dev = ps && ps->device_describe_adaptive(dim, kind_a, f_a, as, sc, od);
      if (adaptive_dev) {
        // an adaptive set (shares that move with the members' outcomes): drawn and adapted on the device, every chain's state
        // starting from its rung's clone (the same bits the host path would start from)
        const int L = as.K + as.K_inner;
        std::vector<double> S((size_t)Ntemps * L), O(S.size()), Wt((size_t)Ntemps * W * L), Th(Wt.size());
        std::vector<int32_t> B((size_t)Ntemps * W * 2), Cn(B.size());
        for (int i = 0; i < Ntemps; i++) {
          std::copy(sc.begin(), sc.end(), S.begin() + (size_t)i * L);
          std::copy(od.begin(), od.end(), O.begin() + (size_t)i * L);
          std::vector<double> w, th;
          std::vector<int> bits, cnt;
          ((proposal_distribution_set*)props[i])->adapt_state(w, th, bits, cnt);
          for (int k = 0; k < W; k++) {
            const size_t c = (size_t)i * W + k;
            std::copy(w.begin(), w.end(), Wt.begin() + c * L);
            std::copy(th.begin(), th.end(), Th.begin() + c * L);
            B[2 * c] = bits[0]; B[2 * c + 1] = bits[1]; Cn[2 * c] = cnt[0]; Cn[2 * c + 1] = cnt[1];
          }
        }
        ptm_check(ptm_set_proposal_adaptive(eng, &as, S.data(), O.data(), Wt.data(), Th.data(), B.data(), Cn.data()), "set_proposal_adaptive");
      } else if (proposal.device_describe_mixture(dim, cum, sc, od)) {   // a proposal_distribution_set of scaled Gaussians
        const int K = (int)cum.size();
        std::vector<double> C((size_t)Ntemps * K), S(C.size()), O(C.size());
        for (int i = 0; i < Ntemps; i++) {
          if (!props[i]->device_describe_mixture(dim, cum, sc, od) || (int)cum.size() != K) { std::cout << "parallel_tempering_chains::set_proposal: rung " << i << "'s clone describes another set" << std::endl; exit(1); }
          for (int k = 0; k < K; k++) { C[(size_t)i * K + k] = cum[k]; S[(size_t)i * K + k] = sc[k]; O[(size_t)i * K + k] = od[k]; }
        }
        ptm_check(ptm_set_proposal_mixture(eng, K, C.data(), S.data(), O.data()), "set_proposal_mixture");
      } else {
        ptm_check(ptm_set_proposal_mixture(eng, 0, nullptr, nullptr, nullptr), "set_proposal_mixture");
      }
      ptm_check(ptm_set_proposal_callback(eng, nullptr, nullptr, nullptr), "set_proposal_callback");
      const int pm = ps ? ps->device_prior_member() : -1;
      prior_dev = pm >= 0;
      if (prior_dev) ptm_check(ptm_set_proposal_prior_draw(eng, pm), "set_proposal_prior_draw");
      ptm_de_params q;
      if (proposal.device_describe_de(q)) {
        // the set's differential evolution is drawn on the device from the device's own history: the extra draws of initialize(n),
        // oldest first (init_x), then the ring
        const size_t N = (size_t)Ntemps * W;
        std::vector<double> rows(init_x.size() * N * dim);
        for (size_t k = 0; k < init_x.size(); k++) std::copy(init_x[k].begin(), init_x[k].end(), rows.begin() + k * N * dim);
        ptm_check(ptm_set_proposal_de(eng, &q, (int)init_x.size(), rows.empty() ? nullptr : rows.data()), "set_proposal_de");
      } else {
        ptm_check(ptm_set_proposal_de(eng, nullptr, 0, nullptr), "set_proposal_de");
      }
      return;
    }
    prior_dev = false;
    if (!host_mode) build_engine(true);   // (initialize() did not know: the engine is set up again, with the same draws)
    for (int w = 0; w < W; w++)
      for (int i = 0; i < Ntemps; i++) {
        proposal_distribution* c = proposal.clone();
        if (c->support_mixing()) c->set_chain(&ladders[w]);
        else c->set_chain(&views[(size_t)w * Ntemps + i]);
        props.push_back(c);   // props[w*Ntemps + i]
      }
    ptm_check(ptm_set_proposal_callback(eng, &parallel_tempering_chains::propose_trampoline, &parallel_tempering_chains::result_trampoline, this),
              "set_proposal_callback");
  }
  bool proposals_on_host() const { return host_mode; }
  bool draws_prior_on_device() const { return prior_dev; }
  bool draws_user_proposal_on_device() const { return user_dev; }
  // Can the device make this proposal's draws from a distribution (draw_from_dist members, device_draw_source)?  Only from the very
  // prior the engine was given as a per-dimension product without a flat dimension (ptm_set_proposal_prior_draw); true without such members
  static bool prior_draws_fit_device(const proposal_distribution& proposal, const sampleable_probability_function* prior, bool prior_on_host) {
    const proposal_distribution_set* ps = dynamic_cast<const proposal_distribution_set*>(&proposal);
    if (!ps) return proposal.device_draw_source() == nullptr;   // (a draw_from_dist on its own: the host's)
    if (ps->prior_draws_need_host()) return false;
    const sampleable_probability_function* src = ps->device_draw_source();
    if (!src) return true;
    if (src != prior || prior_on_host) return false;
    std::vector<int> types;
    std::vector<double> centers, halfwidths;
    if (!prior->describe(types, centers, halfwidths)) return false;
    for (size_t d = 0; d < types.size(); d++) if (types[d] == PTM_PRIOR_FLAT) return false;
    return true;
  }
  bool prior_evaluated_on_host() const { return prior_on_host && !prior_on_device; }   // the prior is not a per-dimension product (describe() == false), and not a device_prior that took the device
  bool prior_evaluated_on_device() const { return prior_on_device; }                  // a device_prior beside a device_likelihood (ptm_set_prior_device)
  std::string step_kernel_name() const { return eng ? std::string(ptm_step_kernel_name(eng)) : std::string(); }   // the kernels a PT step of this ladder runs
  // chain::report_prop (chain.cc:2096-2109 flavour): every rung's proposal report, replica 0
  std::string report_prop(int style = 0) override {
    std::ostringstream ss;
    if (adaptive_dev && !host_mode) {
      // the device's adaptive shares (replica 0) into the rungs' clones, which then report them
      // (the shares are not part of a checkpoint -- as on the host path and in the reference -- and start afresh on a restart)
      const size_t N = (size_t)Ntemps * W;
      std::vector<double> w, th;
      std::vector<int> b0, c0;
      ((proposal_distribution_set*)props[0])->adapt_state(w, th, b0, c0);
      const size_t L = w.size();
      std::vector<double> Wt(N * L), Th(N * L);
      std::vector<int32_t> B(N * 2), Cn(N * 2);
      ptm_check(ptm_batch_begin(eng), "report_prop");
      ptm_check(ptm_get_proposal_adapt_state(eng, Wt.data(), Th.data(), B.data(), Cn.data()), "report_prop");
      ptm_check(ptm_batch_end(eng), "report_prop");
      for (int i = 0; i < Ntemps && i < (int)props.size(); i++) {
        const size_t c = (size_t)i * W;   // (walker 0 of this engine: replica 0)
        ((proposal_distribution_set*)props[i])->set_adapt_state(&Wt[c * L], &Th[c * L], &B[2 * c], &Cn[2 * c]);
      }
    }
    for (int i = 0; i < Ntemps && i < (int)props.size(); i++) ss << "  T=" << 1 / cur_beta(i, 0) << ": " << props[i]->report(style) << "\n";
    return ss.str();
  }
  // per-rung factors for proposals that differ by rung (what user_gaussian_prop's check_update achieves in the reference)
  void set_proposal_factors(int kind, const std::vector<double>& factors, const std::vector<double>& oneDfracs = std::vector<double>()) {
    ptm_check(ptm_set_proposals(eng, kind, factors.data(), oneDfracs.empty() ? nullptr : oneDfracs.data()), "set_proposals");
    dev_prop_kind = kind;
  }
  void step() override { step_in_bins(1, [this](int) { step_one(); }); }
  void step_one() {
    ptm_check(ptm_step(eng, 1), "parallel_tempering_chains::step");
    nstep++;
    fresh = hist_fresh = map_fresh = false;
    if (host_mode || tracking) {   // what the host needs of this step, read with ONE wait on the device
      ptm_check(ptm_batch_begin(eng), "parallel_tempering_chains::step");
      if (host_mode) fetch_history();
      if (tracking) fetch_swaps();
      ptm_check(ptm_batch_end(eng), "parallel_tempering_chains::step");
      if (host_mode) append_history();
      if (tracking) replay_swaps();
    }
  }
  // n steps in ONE engine call when nothing on the host has to look in between (no host-side proposals, no exchange tracking):
  // small ladders then run many steps per kernel launch (ptm_fused_kernel.hpp) instead of paying the launch and the tables'
  // staging for every step.  Same chains as n calls of step().
  void step_n(int n) {
    if (n <= 0) return;
    if (host_mode || tracking) { for (int k = 0; k < n; k++) step(); return; }
    step_in_bins(n, [this](int k) {
      ptm_check(ptm_step(eng, k), "parallel_tempering_chains::step_n");
      nstep += k;
      fresh = hist_fresh = map_fresh = false;
    });
  }
  void step(int n) { step_n(n); }
  double getMAPlpost() override { return views[0].getMAPlpost(); }   // the cold rung's (chain.cc:1570-1571)
  state getMAPstate() override { return views[0].getMAPstate(); }
  state getState(int = -1, bool = false) override { return views[0].getState(); }
  double getLogPost(int = -1, bool = false) override { return views[0].getLogPost(); }
  double getLogLike(int = -1, bool = false) override { return views[0].getLogLike(); }
  int getStep() override { return nstep; }
  int multiplicity() override { return Ntemps; }
  chain* subchain(int index) override { return subchain(index, 0); }
  chain* subchain(int index, int replica) {
    if (index >= 0 && index < Ntemps && replica >= 0 && replica < W) return &views[(size_t)replica * Ntemps + index];
    std::cout << "parallel_tempering_chains::subchain:index out of range. (" << index << " of " << Ntemps << ")" << std::endl;
    exit(1);
  }
  ptm_engine* engine() { return eng; }
  // MH_chain::dumpChain (chain.cc:1112-1135) for rung `ichain`: one line per saved step i = Nburn, Nburn+ievery, ... :
  //   i lpost llike acceptance_ratio prop_type: p0 ... pD-1 invtemp
  // Rows that have already left the ring are skipped (the ring holds the newest rows_per_chain saved states).
  // The device's history ring -> hx / hl / hp / hmeta / hb (the ring's own layout [row][history chain]), the chains a dump or an
  // effective-sample estimate reads: rungs [0, hist_read_rungs) if the driver has said which it writes out (limit_history_reads:
  // ptmcmc_sampler::run dumps pt_dump_n rungs and estimates on the cold one), every history rung as soon as anybody asks beyond.  With
  // differential evolution on the device the ring holds EVERY rung for the whole run: all of it was 0.1 s per output event at 128
  // temperatures x 4000 rows of 32 parameters, most of a run that reports every 500 steps.
  void read_history(size_t at, const char* who) {
    const size_t HC = (size_t)history_rungs() * W, cap = hist_rows;
    size_t want = hist_read_rungs > 0 ? (size_t)std::min(hist_read_rungs, history_rungs()) * W : HC;
    if (at >= want) want = HC;
    if (hist_fresh && hist_have >= want) return;
    hx.resize(cap * HC * dim); hl.resize(cap * HC); hp.resize(cap * HC); hmeta.resize(cap * HC * 4); hnhist.resize((size_t)Ntemps * W); hb.resize(cap * HC);
    ptm_check(ptm_get_history_chains(eng, 0, (int)want, hx.data(), hl.data(), hp.data(), hmeta.data(), hb.data()), who);   // (hb: the temperature each row was saved at)
    ptm_check(ptm_get_array(eng, PTM_ARR_NHIST, hnhist.data()), who);
    hist_fresh = true;
    hist_have = want;
  }
  void limit_history_reads(int rungs) { hist_read_rungs = rungs; }
  void dumpChain(int ichain, std::ostream& os, int Nburn = 0, int ievery = 1, int replica = 0) {
    if (host_mode) {   // host-side proposals: the whole saved history is in the host mirror
      const size_t at = (size_t)ichain * W + replica;
      const mirror_t& m = mirror[at];
      std::vector<int64_t> nh((size_t)Ntemps * W);
      ptm_check(ptm_get_array(eng, PTM_ARR_NHIST, nh.data()), "dumpChain");
      const int Ninit = Ninit_rows, Nhist = (int)nh[at];
      os << "#Ninit=" << Ninit << ", Nburn=" << Nburn << "\n";
      os << "#eval: log(posterior) log(likelihood) acceptance_ratio prop_type: ";
      for (int i = 0; i < dim; i++) os << (sp ? sp->get_name(i) : std::string("[unnamed]")) << " ";
      os << std::endl;
      if (Nburn + Ninit < 0) Nburn = -Ninit;
      const double invtemp = cur_beta(ichain, replica);
      for (int i = Nburn; i < Nhist; i += ievery) {
        int idx = Ninit + i;
        if (i >= 0) idx = Ninit + i / add_every_N;
        if (idx < 0 || (size_t)idx >= m.rows()) continue;
        const double t = m.beta[idx] * m.llike[idx];
        os << i << " " << m.lprior[idx] + t << " " << m.llike[idx] << " " << m.meta[3 * idx] / (double)m.meta[3 * idx + 1] << " " << m.meta[3 * idx + 2] << ": ";
        for (int j = 0; j < dim - 1; j++) os << m.x[(size_t)idx * dim + j] << " ";
        os << m.x[(size_t)idx * dim + dim - 1] << " " << invtemp << std::endl;
      }
      return;
    }
    if (hist_rows <= 0) { std::cout << "parallel_tempering_chains::dumpChain: call keep_history(rows) before initialize()" << std::endl; exit(1); }
    if (ichain >= history_rungs()) { std::cout << "parallel_tempering_chains::dumpChain: rung " << ichain << " keeps no history (keep_history(rows, " << history_rungs() << "))" << std::endl; exit(1); }
    const size_t HC = (size_t)history_rungs() * W, cap = hist_rows, at = (size_t)ichain * W + replica;
    read_history(at, "dumpChain");   // one read-back serves every rung / replica dumped at this step
    const std::vector<int32_t>& meta = hmeta;
    // (rows are numbered as the ring numbers them -- row 0 the start state --; with differential evolution on the device the header
    //  names the initial draws the device keeps beside the ring, as the reference's file does)
    const int Ninit = 1, Nhist = (int)hnhist[at];
    os << "#Ninit=" << (de_built ? Ninit_asked : Ninit) << ", Nburn=" << Nburn << "\n";
    os << "#eval: log(posterior) log(likelihood) acceptance_ratio prop_type: ";
    for (int i = 0; i < dim; i++) os << (sp ? sp->get_name(i) : std::string("[unnamed]")) << " ";
    os << std::endl;
    const int Nfront = de_built ? Ninit_asked - 1 : 0;              // initial draws in front of the ring's row 0 (kept by the host too: init_x)
    if (Nburn + Ninit + Nfront < 0) Nburn = -(Ninit + Nfront);
    const double invtemp = cur_beta(ichain, replica);   // the chain's CURRENT temperature on every row (chain.cc:1131)
    for (int i = Nburn; i < Nhist; i += ievery) {
      if (i + Ninit < 0) {   // one of the initial draws in front of the start state (MH_chain::initialize adds every one, chain.cc:846-876)
        const int k = Nfront + Ninit + i;
        if (k < 0 || k >= (int)init_x.size()) continue;
        const double t = (1 / temps[ichain]) * init_ll[k][at];
        os << i << " " << init_lp[k][at] + t << " " << init_ll[k][at] << " " << 1.0 << " " << -1 << ": ";
        for (int j = 0; j < dim - 1; j++) os << init_x[k][at * dim + j] << " ";
        os << init_x[k][at * dim + dim - 1] << " " << invtemp << std::endl;
        continue;
      }
      int idx = Ninit + i;                                          // chain.cc:1124-1125
      if (i >= 0) idx = Ninit + i / add_every_N;                    // get_state_idx, chain.cc:1041-1050 (Nzero = 0)
      const size_t o = (size_t)(idx % (int)cap) * HC + at;
      if (idx < 0 || meta[4 * o + 3] != idx) continue;              // not saved yet / overwritten in the ring
      const double lpo = hp[o] + hb[o] * hl[o];                     // chain.cc:928, at the temperature of that add_state
      os << i << " " << lpo << " " << hl[o] << " " << meta[4 * o] / (double)meta[4 * o + 1] << " " << meta[4 * o + 2] << ": ";
      for (int j = 0; j < dim - 1; j++) os << hx[o * dim + j] << " ";
      os << hx[o * dim + dim - 1];
      os << " " << invtemp;
      os << std::endl;
    }
  }
  // ---- effective sample size of the cold chain (chain::report_effective_samples, chain.cc:457-643; the sampler's
  // chain_ess_stop criterion, ptmcmc.cc:628-649): ess_estimator (above) on the cold chain's saved history, the first 20
  // parameters as features.  Returns (ess, useful chain length).  Needs the cold chain's whole saved history: the host mirror
  // (host-side proposals) or a history ring as long as the run (keep_history).
  bool cold_row(int step, std::vector<double>& out, int replica = 0) {   // state the cold chain saved for nominal step `step`
    const size_t at = (size_t)replica;
    if (step < 0) return false;
    if (host_mode) {
      const mirror_t& m = mirror[at];
      const size_t r = (size_t)Ninit_rows + step / add_every_N;
      if (r >= m.rows()) return false;
      out.assign(m.x.begin() + r * dim, m.x.begin() + (r + 1) * dim);
      return true;
    }
    if (hist_rows <= 0) return false;
    const size_t HC = (size_t)history_rungs() * W, cap = hist_rows;
    read_history(at, "report_effective_samples");
    const int idx = 1 + step / add_every_N;
    const size_t o = (size_t)(idx % (int)cap) * HC + at;
    if (hmeta[4 * o + 3] != idx) return false;
    out.assign(hx.begin() + o * dim, hx.begin() + (o + 1) * dim);
    return true;
  }
  int cold_steps(int replica = 0) {   // MH_chain::getStep() of the cold chain: its add_state calls
    std::vector<int64_t> nh((size_t)Ntemps * W);
    ptm_check(ptm_get_array(eng, PTM_ARR_NHIST, nh.data()), "report_effective_samples");
    return (int)nh[(size_t)replica];
  }
  // The device estimates from its own ring (ptm_ess_*: every replica at once, each with its own count of add_state calls, the host
  // estimator's bits) when the ring is there; with host-side proposals (the history is the host mirror) and with PTM_HOST_ESS=1 the
  // estimate is made here.
  bool ess_on_device_possible() {
    static const bool off = [] { const char* v = getenv("PTM_HOST_ESS"); return v && *v && *v != '0'; }();   // (A/B: keep the host path)
    return !(off || host_mode || hist_rows <= 0);
  }
  int ess_features(int imax) const {
    if (imax < 0 || imax > dim) imax = dim;
    return imax > 20 ? 20 : imax;   // (the reference's simplified interface looks at the first 20 parameters)
  }
  std::pair<double, int> report_effective_samples(int imax = -1, int width = 40000, int every = 100, double esslimit = -1, bool reporting = true) {
    const int nf = ess_features(imax);
    ess_estimator est(cold_steps(), nf, [this](int step, std::vector<double>& row) { return cold_row(step, row); });
    ess_dev_last = false;
    if (ess_on_device_possible())
      est.use_backend([this, nf](int width, int every, int burn, double& ess, int& nwin) {
        std::vector<double> e((size_t)W);
        std::vector<int32_t> n((size_t)W);
        ptm_check(ptm_ess_windowed(eng, 0, nf, width, every, burn, e.data(), n.data()), "report_effective_samples");
        if (ptm_ess_last_on_device(eng)) ess_dev_last = true;   // (a pass of the search too short for one window launches nothing)
        ess = e[0]; nwin = n[0];
      });
    const std::pair<double, int> r = est.report(width, every, esslimit, views.empty() ? 0 : views[0].size(), Ninit_rows);
    if (reporting) print_effective_samples(imax, r);
    return r;
  }
  void print_effective_samples(int imax, const std::pair<double, int>& r) {
    std::cout << "Over " << ess_features(imax) << " pars: ess=" << r.first << "  useful chain length is: " << r.second << " autocorrlen=" << (r.first > 0 ? r.second / r.first : 0.0) << std::endl;
  }
  // the same for every replica of this process: (ess, useful chain length) of each cold chain
  std::vector<std::pair<double, int> > report_effective_samples_all(int imax = -1, int width = 40000, int every = 100, double esslimit = -1) {
    const int nf = ess_features(imax);
    std::vector<std::pair<double, int> > out((size_t)W);
    if (ess_on_device_possible() && width >= 1) {
      if (every < 0) {   // the stride the series was saved with (ess_estimator::report)
        const int rows = views.empty() ? 0 : views[0].size();
        every = rows > Ninit_rows ? (int)(0.5 + ((double)cold_steps() - Ninit_rows) / (rows - Ninit_rows)) : 1;
      }
      if (every < 1) every = 1;
      std::vector<double> e((size_t)W);
      std::vector<int32_t> len((size_t)W);
      ptm_check(ptm_ess_report(eng, 0, nf, width, every, esslimit, e.data(), len.data()), "report_effective_samples_all");
      ess_dev_last = ptm_ess_last_on_device(eng) != 0;
      for (int w = 0; w < W; w++) out[(size_t)w] = std::make_pair(e[(size_t)w], (int)len[(size_t)w]);
      return out;
    }
    ess_dev_last = false;
    for (int w = 0; w < W; w++) {
      ess_estimator est(cold_steps(w), nf, [this, w](int step, std::vector<double>& row) { return cold_row(step, row, w); });
      out[(size_t)w] = est.report(width, every, esslimit, views.empty() ? 0 : views[0].size(), Ninit_rows);
    }
    return out;
  }
  bool ess_dev_last = false;
  bool ess_ran_on_device() const { return ess_dev_last; }   // the last estimate of this ladder launched the device's kernels
  // ---- split R-hat across the replicas of rung `rung` (rhat_estimator above; no reference counterpart: it runs one ladder): every
  // replica's newest `nrows` saved rows (even, >= 4), the first `nfeat` parameters.  The device estimates from its own ring (ptm_rhat:
  // the host estimator's bits) when the ring is there; with host-side proposals (the history is the host mirror) and with
  // PTM_HOST_RHAT=1 the estimate is made here.
  bool rhat_on_device_possible() {
    static const bool off = [] { const char* v = getenv("PTM_HOST_RHAT"); return v && *v && *v != '0'; }();   // (A/B: keep the host path)
    return !(off || host_mode || hist_rows <= 0);
  }
  // the saved rows behind the start state that every replica of the rung has, and the ring still holds
  int rhat_rows_available(int rung = 0) {
    std::vector<int64_t> nh((size_t)Ntemps * W);
    ptm_check(ptm_get_array(eng, PTM_ARR_NHIST, nh.data()), "split_rhat");
    long long have = -1;
    for (int w = 0; w < W; w++) {
      const long long st = nh[(size_t)rung * W + w], newest = st > 0 ? rhat_estimator::newest_row(st, add_every_N) : 0;
      if (have < 0 || newest < have) have = newest;
    }
    if (!host_mode && have > hist_rows) have = hist_rows;
    return (int)have;
  }
  rhat_estimator::result split_rhat(int rung = 0, int nfeat = -1, int nrows = -1) {
    if (nfeat < 0 || nfeat > dim) nfeat = dim;
    if (nrows < 0) { nrows = rhat_rows_available(rung); nrows -= nrows % 2; }
    rhat_dev_last = false;
    rhat_estimator::result r;
    if (rhat_on_device_possible()) {
      const size_t nf = (size_t)(nfeat > 0 ? nfeat : 0), ns = 2 * (size_t)W * nf;
      r.rhat.assign(nf, 0.0); r.mean = r.rhat; r.within = r.rhat; r.between = r.rhat;
      r.seq_mean.assign(ns, 0.0); r.seq_var = r.seq_mean;
      ptm_check(ptm_rhat(eng, rung, nfeat, nrows, r.rhat.data(), r.mean.data(), r.within.data(), r.between.data(), r.seq_mean.data(), r.seq_var.data()), "split_rhat");
      r.complete = true;
      rhat_dev_last = true;
      return r;
    }
    if (rung < 0 || rung >= (host_mode ? Ntemps : history_rungs()) || nfeat < 1 || nrows < 4 || nrows % 2) {
      std::cout << "parallel_tempering_chains::split_rhat: rung " << rung << ", nfeat " << nfeat << ", nrows " << nrows << " (a recorded rung, 1..dim, even and >= 4)" << std::endl;
      exit(1);
    }
    std::vector<int64_t> nh((size_t)Ntemps * W);
    ptm_check(ptm_get_array(eng, PTM_ARR_NHIST, nh.data()), "split_rhat");
    std::vector<long long> newest((size_t)W);
    for (int w = 0; w < W; w++) {
      const long long st = nh[(size_t)rung * W + w];
      newest[(size_t)w] = st > 0 ? rhat_estimator::newest_row(st, add_every_N) : 0;
      if (newest[(size_t)w] < nrows) { std::cout << "parallel_tempering_chains::split_rhat: replica " << w << " has saved " << newest[(size_t)w] << " rows behind its start state, fewer than nrows (" << nrows << ")" << std::endl; exit(1); }
    }
    rhat_estimator::reader read;
    if (host_mode) read = [this, rung](int w, long long row, std::vector<double>& v) {   // (the mirror counts its initial draws in front)
      const mirror_t& m = mirror[(size_t)rung * W + w];
      const long long at = row - 1 + Ninit_rows;
      if (row < 1 || (size_t)at >= m.rows()) return false;
      v.assign(m.x.begin() + (size_t)at * dim, m.x.begin() + ((size_t)at + 1) * dim);
      return true;
    };
    else {
      read_history((size_t)rung * W + W - 1, "split_rhat");
      read = [this, rung](int w, long long row, std::vector<double>& v) {
        const size_t HC = (size_t)history_rungs() * W, cap = hist_rows;
        const size_t o = (size_t)(row % (long long)cap) * HC + (size_t)rung * W + w;
        if (row < 1 || hmeta[4 * o + 3] != (int32_t)row) return false;
        v.assign(hx.begin() + o * dim, hx.begin() + (o + 1) * dim);
        return true;
      };
    }
    r = rhat_estimator::estimate(W, nfeat, nrows, newest.data(), read);
    if (!r.complete) { std::cout << "parallel_tempering_chains::split_rhat: the saved history no longer holds the window (" << nrows << " rows)" << std::endl; exit(1); }
    return r;
  }
  bool rhat_dev_last = false;
  bool rhat_ran_on_device() const { return rhat_dev_last; }   // the last split_rhat of this ladder ran the device's kernels
  // ---- pooled posterior mean and covariance over the replicas of rung `rung` (moments_estimator above; the reference's covariance
  // reader and writer are empty): every replica's newest `nrows` saved rows (< 0: all that every replica has), the first `nfeat`
  // parameters.  The device estimates from its own ring (ptm_moments: the host estimator's bits) when the ring is there; with
  // host-side proposals (the history is the host mirror) and with PTM_HOST_MOMENTS=1 the estimate is made here.  Above 128
  // parameters the mean and the variances alone (result::cov stays empty).
  bool moments_on_device_possible() {
    static const bool off = [] { const char* v = getenv("PTM_HOST_MOMENTS"); return v && *v && *v != '0'; }();   // (A/B: keep the host path)
    return !(off || host_mode || hist_rows <= 0);
  }
  moments_estimator::result posterior_moments(int rung = 0, int nfeat = -1, int nrows = -1) {
    if (nfeat < 0 || nfeat > dim) nfeat = dim;
    if (nrows < 0) nrows = rhat_rows_available(rung);
    const bool want_cov = nfeat <= 128;
    moments_dev_last = false;
    moments_estimator::result r;
    if (moments_on_device_possible()) {
      const size_t nf = (size_t)(nfeat > 0 ? nfeat : 0);
      r.nfeat = nfeat; r.count = 0;
      r.mean.assign(nf, 0.0); r.var = r.mean;
      if (want_cov) r.cov.assign(nf * nf, 0.0);
      r.walker_sum.assign((size_t)W * nf, 0.0);
      int64_t count = 0;
      ptm_check(ptm_moments(eng, rung, nfeat, nrows, r.mean.data(), want_cov ? r.cov.data() : nullptr, r.var.data(), r.walker_sum.data(), &count), "posterior_moments");
      r.count = count;
      r.complete = true;
      moments_dev_last = true;
      return r;
    }
    if (rung < 0 || rung >= (host_mode ? Ntemps : history_rungs()) || nfeat < 1 || nrows < 1 || (long long)W * nrows < 2) {
      std::cout << "parallel_tempering_chains::posterior_moments: rung " << rung << ", nfeat " << nfeat << ", nrows " << nrows << " (a recorded rung, 1..dim, at least 1 and two samples in all)" << std::endl;
      exit(1);
    }
    std::vector<int64_t> nh((size_t)Ntemps * W);
    ptm_check(ptm_get_array(eng, PTM_ARR_NHIST, nh.data()), "posterior_moments");
    std::vector<long long> newest((size_t)W);
    for (int w = 0; w < W; w++) {
      const long long st = nh[(size_t)rung * W + w];
      newest[(size_t)w] = st > 0 ? rhat_estimator::newest_row(st, add_every_N) : 0;
      if (newest[(size_t)w] < nrows) { std::cout << "parallel_tempering_chains::posterior_moments: replica " << w << " has saved " << newest[(size_t)w] << " rows behind its start state, fewer than nrows (" << nrows << ")" << std::endl; exit(1); }
    }
    moments_estimator::reader read;
    if (host_mode) read = [this, rung](int w, long long row, std::vector<double>& v) {   // (the mirror counts its initial draws in front)
      const mirror_t& m = mirror[(size_t)rung * W + w];
      const long long at = row - 1 + Ninit_rows;
      if (row < 1 || (size_t)at >= m.rows()) return false;
      v.assign(m.x.begin() + (size_t)at * dim, m.x.begin() + ((size_t)at + 1) * dim);
      return true;
    };
    else {
      read_history((size_t)rung * W + W - 1, "posterior_moments");
      read = [this, rung](int w, long long row, std::vector<double>& v) {
        const size_t HC = (size_t)history_rungs() * W, cap = hist_rows;
        const size_t o = (size_t)(row % (long long)cap) * HC + (size_t)rung * W + w;
        if (row < 1 || hmeta[4 * o + 3] != (int32_t)row) return false;
        v.assign(hx.begin() + o * dim, hx.begin() + (o + 1) * dim);
        return true;
      };
    }
    r = moments_estimator::estimate(W, nfeat, nrows, newest.data(), read, want_cov);
    if (!r.complete) { std::cout << "parallel_tempering_chains::posterior_moments: the saved history no longer holds the window (" << nrows << " rows)" << std::endl; exit(1); }
    return r;
  }
  bool moments_dev_last = false;
  bool moments_ran_on_device() const { return moments_dev_last; }   // the last posterior_moments of this ladder ran the device's kernels
  // ---- every recorded rung's Gaussian factor from that rung's own samples (what user_gaussian_prop::check_update / reset_dist do for
  // one chain in the reference, proposal_distribution.cc:340-441): every replica's newest `nrows` saved rows (< 0: the largest window
  // every replica of every recorded rung has), factor = scale * eigen_factor(pooled covariance) (DENSE) or sigma = scale * sqrt(var)
  // (DIAG); scale <= 0: 2.38 / sqrt(dim).  A rung whose covariance is not finite or not positive definite keeps its factor.  The
  // device does all of it in one call (ptm_adapt_proposals); with PTM_HOST_PROPOSAL_ADAPT=1 the host route runs instead --
  // posterior_moments of every rung, gaussian_prop::eigen_factor, ptm_set_proposal_rung -- and gives the same bits.  With host-side or
  // device user proposals, a Cholesky factor or no ring nothing is adapted (said once).  Returns the rungs that were set.
  struct proposal_adapt_result { int rows = 0, rungs = 0, set = 0, not_finite = 0, not_positive = 0; };
  bool proposal_adapt_on_device_possible() {
    static const bool off = [] { const char* v = getenv("PTM_HOST_PROPOSAL_ADAPT"); return v && *v && *v != '0'; }();   // (A/B: keep the host route)
    return !(off || host_mode || hist_rows <= 0);
  }
  proposal_adapt_result adapt_gaussian_proposals(int nrows = -1, double scale = -1.0) {
    proposal_adapt_result res;
    proposal_adapt_dev_last = false;
    const int nr = history_rungs();
    const char* why = host_mode ? "the proposals are drawn on the host" : user_dev ? "the proposals are a device_proposal's" : dev_prop_kind < 0 ? "no Gaussian factors are set" :
                      dev_prop_kind == PTM_PROP_LOWER ? "the factors are Cholesky factors" : (dev_prop_kind == PTM_PROP_DENSE && dim > 128) ? "dense factors are adapted up to 128 parameters" :
                      nr <= 0 ? "no history is kept" : nullptr;
    if (why) {
      if (!proposal_adapt_said) std::cout << "parallel_tempering_chains::adapt_gaussian_proposals: nothing is adapted (" << why << ")" << std::endl;
      proposal_adapt_said = true;
      return res;
    }
    if (!(scale > 0)) scale = 2.38 / std::sqrt((double)dim);
    if (nrows < 0) {
      std::vector<int64_t> nh((size_t)Ntemps * W);
      ptm_check(ptm_get_array(eng, PTM_ARR_NHIST, nh.data()), "adapt_gaussian_proposals");
      long long have = -1;
      for (size_t c = 0; c < (size_t)nr * W; c++) {
        const long long newest = nh[c] > 0 ? rhat_estimator::newest_row(nh[c], add_every_N) : 0;
        if (have < 0 || newest < have) have = newest;
      }
      if (have > hist_rows) have = hist_rows;
      nrows = (int)have;
    }
    res.rows = nrows; res.rungs = nr;
    std::vector<int32_t> status((size_t)nr, 0);
    if (proposal_adapt_on_device_possible()) {
      ptm_check(ptm_adapt_proposals(eng, 0, nr, nrows, scale, status.data(), nullptr), "adapt_gaussian_proposals");
      proposal_adapt_dev_last = true;
    } else {
      const bool diag = dev_prop_kind == PTM_PROP_DIAG;
      for (int r = 0; r < nr; r++) {
        const moments_estimator::result m = posterior_moments(r, dim, nrows);
        const std::vector<double>& in = diag ? m.var : m.cov;
        bool finite = true;
        for (size_t k = 0; k < in.size(); k++) finite = finite && std::isfinite(in[k]);
        std::vector<double> f;
        bool positive = true;
        if (diag) {
          f.resize((size_t)dim);
          for (int d = 0; d < dim; d++) { positive = positive && m.var[(size_t)d] > 0; f[(size_t)d] = scale * std::sqrt(m.var[(size_t)d]); }
        } else {
          std::vector<double> lam;
          gaussian_prop::eigen_factor(m.cov, dim, f, &lam);
          for (size_t k = 0; k < f.size(); k++) f[k] = scale * f[k];
          positive = lam[0] > 0;
        }
        status[(size_t)r] = !finite ? 1 : (positive ? 0 : 2);
        if (status[(size_t)r] == 0) ptm_check(ptm_set_proposal_rung(eng, r, f.data(), -1.0), "adapt_gaussian_proposals");
      }
    }
    for (int r = 0; r < nr; r++) { res.set += status[(size_t)r] == 0; res.not_finite += status[(size_t)r] == 1; res.not_positive += status[(size_t)r] == 2; }
    return res;
  }
  bool proposal_adapt_dev_last = false, proposal_adapt_said = false;
  int dev_prop_kind = -1;   // the kind of the factors on the device (ptm_set_proposals), -1: none
  bool proposal_adapt_ran_on_device() const { return proposal_adapt_dev_last; }   // the last adapt_gaussian_proposals ran the device's kernels
  // ---- exact pooled quantiles over the replicas of rung `rung` (quantile_estimator above): every replica's newest `nrows` saved
  // rows (< 0: all that every replica has), the first `nfeat` parameters, at the probabilities `probs`.  The device selects from its
  // own ring (ptm_quantiles: the host estimator's bits) when the ring is there; with host-side proposals (the history is the host
  // mirror) and with PTM_HOST_QUANTILES=1 the estimate is made here.
  bool quantiles_on_device_possible() {
    static const bool off = [] { const char* v = getenv("PTM_HOST_QUANTILES"); return v && *v && *v != '0'; }();   // (A/B: keep the host path)
    return !(off || host_mode || hist_rows <= 0);
  }
  quantile_estimator::result posterior_quantiles(const std::vector<double>& probs, int rung = 0, int nfeat = -1, int nrows = -1) {
    if (nfeat < 0 || nfeat > dim) nfeat = dim;
    if (nrows < 0) nrows = rhat_rows_available(rung);
    quantiles_dev_last = false;
    quantile_estimator::result r;
    if (quantiles_on_device_possible()) {
      const size_t nf = (size_t)(nfeat > 0 ? nfeat : 0);
      r.nfeat = nfeat; r.count = 0; r.probs = probs;
      r.q.assign(probs.size() * nf, 0.0); r.x_lo = r.q; r.x_hi = r.q;
      int64_t count = 0;
      ptm_check(ptm_quantiles(eng, rung, nfeat, nrows, (int)probs.size(), probs.data(), r.q.data(), r.x_lo.data(), r.x_hi.data(), &count), "posterior_quantiles");
      r.count = count;
      r.complete = true;
      quantiles_dev_last = true;
      return r;
    }
    bool probs_ok = !probs.empty() && probs.size() <= 32;
    for (size_t k = 0; k < probs.size(); k++) probs_ok = probs_ok && probs[k] >= 0.0 && probs[k] <= 1.0;
    if (rung < 0 || rung >= (host_mode ? Ntemps : history_rungs()) || nfeat < 1 || nrows < 1 || !probs_ok) {
      std::cout << "parallel_tempering_chains::posterior_quantiles: rung " << rung << ", nfeat " << nfeat << ", nrows " << nrows << ", " << probs.size() << " probabilities (a recorded rung, 1..dim, at least 1, 1..32 values in [0, 1])" << std::endl;
      exit(1);
    }
    std::vector<int64_t> nh((size_t)Ntemps * W);
    ptm_check(ptm_get_array(eng, PTM_ARR_NHIST, nh.data()), "posterior_quantiles");
    std::vector<long long> newest((size_t)W);
    for (int w = 0; w < W; w++) {
      const long long st = nh[(size_t)rung * W + w];
      newest[(size_t)w] = st > 0 ? rhat_estimator::newest_row(st, add_every_N) : 0;
      if (newest[(size_t)w] < nrows) { std::cout << "parallel_tempering_chains::posterior_quantiles: replica " << w << " has saved " << newest[(size_t)w] << " rows behind its start state, fewer than nrows (" << nrows << ")" << std::endl; exit(1); }
    }
    quantile_estimator::reader read;
    if (host_mode) read = [this, rung](int w, long long row, std::vector<double>& v) {   // (the mirror counts its initial draws in front)
      const mirror_t& m = mirror[(size_t)rung * W + w];
      const long long at = row - 1 + Ninit_rows;
      if (row < 1 || (size_t)at >= m.rows()) return false;
      v.assign(m.x.begin() + (size_t)at * dim, m.x.begin() + ((size_t)at + 1) * dim);
      return true;
    };
    else {
      read_history((size_t)rung * W + W - 1, "posterior_quantiles");
      read = [this, rung](int w, long long row, std::vector<double>& v) {
        const size_t HC = (size_t)history_rungs() * W, cap = hist_rows;
        const size_t o = (size_t)(row % (long long)cap) * HC + (size_t)rung * W + w;
        if (row < 1 || hmeta[4 * o + 3] != (int32_t)row) return false;
        v.assign(hx.begin() + o * dim, hx.begin() + (o + 1) * dim);
        return true;
      };
    }
    r = quantile_estimator::estimate(W, nfeat, nrows, newest.data(), read, probs);
    if (!r.complete) { std::cout << "parallel_tempering_chains::posterior_quantiles: the saved history no longer holds the window (" << nrows << " rows)" << std::endl; exit(1); }
    return r;
  }
  bool quantiles_dev_last = false;
  bool quantiles_ran_on_device() const { return quantiles_dev_last; }   // the last posterior_quantiles of this ladder ran the device's kernels
  // ---- the corner plot's counts over the replicas of rung `rung` (histogram_estimator above): every replica's newest `nrows` saved
  // rows (< 0: all that every replica has), the first `nfeat` parameters, nbins bins between lo[f] and hi[f]; pairs: the 2-D
  // histograms too.  The device counts on its own ring (ptm_histograms: the host estimator's integers) when the ring is there; with
  // host-side proposals (the history is the host mirror) and with PTM_HOST_HISTOGRAMS=1 the counting is done here.
  bool histograms_on_device_possible() {
    static const bool off = [] { const char* v = getenv("PTM_HOST_HISTOGRAMS"); return v && *v && *v != '0'; }();   // (A/B: keep the host path)
    return !(off || host_mode || hist_rows <= 0);
  }
  histogram_estimator::result posterior_histograms(const std::vector<double>& lo, const std::vector<double>& hi, int nbins, int rung = 0, int nfeat = -1, int nrows = -1,
                                                   bool pairs = true) {
    if (nfeat < 0 || nfeat > dim) nfeat = dim;
    if (nrows < 0) nrows = rhat_rows_available(rung);
    histograms_dev_last = false;
    const size_t nf = (size_t)(nfeat > 0 ? nfeat : 0);
    if (lo.size() < nf || hi.size() < nf) {
      std::cout << "parallel_tempering_chains::posterior_histograms: lo and hi must hold a value for each of the " << nf << " parameters" << std::endl;
      exit(1);
    }
    histogram_estimator::result r;
    if (histograms_on_device_possible()) {
      const size_t nb = (size_t)(nbins > 0 && nbins <= 128 ? nbins : 0), np = pairs && nf > 1 ? histogram_estimator::npairs(nfeat) : 0;
      r.nfeat = nfeat; r.nbins = nbins; r.lo.assign(lo.begin(), lo.begin() + nf); r.hi.assign(hi.begin(), hi.begin() + nf);
      r.h1.assign(nf * nb, 0); r.below.assign(nf, 0); r.above.assign(nf, 0);
      if ((double)np * nb * nb <= 33554432.0) r.h2.assign(np * nb * nb, 0);   // (more than that is refused by the call)
      int64_t count = 0, none = 0;
      ptm_check(ptm_histograms(eng, rung, nfeat, nrows, nbins, lo.data(), hi.data(), r.h1.data(), pairs ? (r.h2.empty() ? &none : r.h2.data()) : nullptr, r.below.data(),
                               r.above.data(), &count), "posterior_histograms");
      r.count = count;
      r.complete = true;
      histograms_dev_last = true;
      return r;
    }
    if (rung < 0 || rung >= (host_mode ? Ntemps : history_rungs()) || nfeat < 1 || nrows < 1 || nbins < 1 || nbins > 128) {
      std::cout << "parallel_tempering_chains::posterior_histograms: rung " << rung << ", nfeat " << nfeat << ", nrows " << nrows << ", " << nbins << " bins (a recorded rung, 1..dim, at least 1, 1..128)" << std::endl;
      exit(1);
    }
    for (size_t f = 0; f < nf; f++)
      if (!histogram_estimator::edges_ok(lo[f], hi[f], nbins)) {
        char buf[120];
        snprintf(buf, sizeof buf, "%.17g to %.17g", lo[f], hi[f]);
        std::cout << "parallel_tempering_chains::posterior_histograms: the range cannot hold nbins bins (parameter " << f << ": " << nbins + 1 << " edges from " << buf << " are not finite and strictly increasing)" << std::endl;
        exit(1);
      }
    if (pairs && (double)histogram_estimator::npairs(nfeat) * nbins * nbins > 33554432.0) {
      std::cout << "parallel_tempering_chains::posterior_histograms: " << nfeat << " parameters and " << nbins << " bins need more than 2^25 pair counters" << std::endl;
      exit(1);
    }
    std::vector<int64_t> nh((size_t)Ntemps * W);
    ptm_check(ptm_get_array(eng, PTM_ARR_NHIST, nh.data()), "posterior_histograms");
    std::vector<long long> newest((size_t)W);
    for (int w = 0; w < W; w++) {
      const long long st = nh[(size_t)rung * W + w];
      newest[(size_t)w] = st > 0 ? rhat_estimator::newest_row(st, add_every_N) : 0;
      if (newest[(size_t)w] < nrows) { std::cout << "parallel_tempering_chains::posterior_histograms: replica " << w << " has saved " << newest[(size_t)w] << " rows behind its start state, fewer than nrows (" << nrows << ")" << std::endl; exit(1); }
    }
    histogram_estimator::reader read;
    if (host_mode) read = [this, rung](int w, long long row, std::vector<double>& v) {   // (the mirror counts its initial draws in front)
      const mirror_t& m = mirror[(size_t)rung * W + w];
      const long long at = row - 1 + Ninit_rows;
      if (row < 1 || (size_t)at >= m.rows()) return false;
      v.assign(m.x.begin() + (size_t)at * dim, m.x.begin() + ((size_t)at + 1) * dim);
      return true;
    };
    else {
      read_history((size_t)rung * W + W - 1, "posterior_histograms");
      read = [this, rung](int w, long long row, std::vector<double>& v) {
        const size_t HC = (size_t)history_rungs() * W, cap = hist_rows;
        const size_t o = (size_t)(row % (long long)cap) * HC + (size_t)rung * W + w;
        if (row < 1 || hmeta[4 * o + 3] != (int32_t)row) return false;
        v.assign(hx.begin() + o * dim, hx.begin() + (o + 1) * dim);
        return true;
      };
    }
    r = histogram_estimator::estimate(W, nfeat, nrows, newest.data(), read, std::vector<double>(lo.begin(), lo.begin() + nf), std::vector<double>(hi.begin(), hi.begin() + nf), nbins, pairs && nfeat > 1);
    if (!r.complete) { std::cout << "parallel_tempering_chains::posterior_histograms: the saved history no longer holds the window (" << nrows << " rows)" << std::endl; exit(1); }
    return r;
  }
  bool histograms_dev_last = false;
  bool histograms_ran_on_device() const { return histograms_dev_last; }   // the last posterior_histograms of this ladder ran the device's kernels
  // swap_count / swap_accept_count (chain.hh:244-245)
  void swap_counts(std::vector<int64_t>& tries, std::vector<int64_t>& accepts) {
    std::vector<int64_t> t((size_t)W * (Ntemps > 1 ? Ntemps - 1 : 1)), a(t.size());
    ptm_check(ptm_get_swap_counts(eng, t.data(), a.data()), "swap_counts");
    tries.assign(t.begin(), t.begin() + (Ntemps > 1 ? Ntemps - 1 : 1));       // replica 0
    accepts.assign(a.begin(), a.begin() + (Ntemps > 1 ? Ntemps - 1 : 1));
  }
  std::string status() override {  // chain.cc:2053-2094 flavour
    refresh();
    std::vector<int32_t> nt((size_t)Ntemps * W), na((size_t)Ntemps * W);
    ptm_get_array(eng, PTM_ARR_NTRIES, nt.data());
    ptm_get_array(eng, PTM_ARR_NACCEPT, na.data());
    std::ostringstream s;
    for (int i = 0; i < Ntemps; i++) {   // replica 0
      const size_t c = (size_t)i * W;
      s << "T=" << 1 / cur_beta(i, 0) << ": lpost=" << lpost[c] << " llike=" << llike[c] << " acc=" << (double)na[c] / nt[c] << "\n";
      if (do_evid && verbose_evid && i < Ntemps - 1 && !ev_up.empty())   // chain.cc:2065
        s << " log eratio:(" << ev_down[(size_t)i * W] << "," << ev_up[(size_t)i * W] << ")" << std::endl;
    }
    if (do_evid) s << "Best evidence stderr=" << bestEvidenceErr() << std::endl;   // chain.cc:2092
    return s.str();
  }
  // MH_chain::dumpChain row format of the current state (chain.cc:1112-1135): i lpost llike acc type: params invtemp
  void dumpCurrent(int ichain, std::ostream& os, int replica = 0) {
    refresh();
    std::vector<int32_t> nt((size_t)Ntemps * W), na((size_t)Ntemps * W), ty((size_t)Ntemps * W);
    ptm_get_array(eng, PTM_ARR_NTRIES, nt.data());
    ptm_get_array(eng, PTM_ARR_NACCEPT, na.data());
    ptm_get_array(eng, PTM_ARR_LAST_TYPE, ty.data());
    const size_t c = (size_t)ichain * W + replica;
    os << nstep << " " << lpost[c] << " " << llike[c] << " " << (double)na[c] / nt[c] << " " << ty[c] << ": ";
    for (int j = 0; j < dim; j++) os << X[c * dim + j] << " ";
    os << cur_beta(ichain, replica) << std::endl;
  }
};

// ---- bayesian.hh:795-821 / ptmcmc.hh: the driver ------------------------------------------------------------------------------
// ---- the proposal test (test_proposal.hh:51-348) ----------------------------------------------------------------------------------
// proposal_tester: does a proposal leave a known target invariant?  N samples of the target are moved by Metropolis-Hastings steps of
// the proposal until ncyc * N moves have been accepted; the transformed set is then compared with the start set and with a fresh draw
// by kl_estimator's two statistics, each calibrated on redraws of the target (kl_verdict).  The transform is what the engine does: the
// samples are the Nsamp replicas of a one-rung ladder whose prior is the target -- a per-dimension product such as
// gaussian_dist_product on the tested space -- over a constant likelihood, with the prior gate out of the way; the ladder installs the
// proposal as it does for a run (Gaussian sets natively, a device_proposal through ptm_set_proposal_device, anything else through
// the host-proposal callback), draws the samples and the redraws (redrawn until valid: the reference's rejection loop, :90-113) and
// counts the acceptances.  The KL estimate always uses EXACT neighbours, searched on the device (ptm_nn_dist2: the host estimator's
// bits; PTM_HOST_KL=1 and more than 128 dimensions: kl_estimator itself).  hastings_err, the reference's way to force a failure, is
// added where the host adds the ratio: it needs a host-side proposal.  A differential_evolution is skipped: the reference hands it an
// empty chain and cannot draw from it.  The proposal's own intrinsic test (involutions) is out of scope.
class proposal_tester {
  proposal_distribution* proposal;
  sampleable_probability_function* target_dist;
  bool loop;
  std::string path;
  uint64_t seed;

  // the proposal with hastings_err added to its ratio (host side only: it describes nothing to the device)
  class with_hastings_err : public proposal_distribution {
    proposal_distribution* inner;
    double err;

   public:
    with_hastings_err(const proposal_distribution& p, double err) : inner(p.clone()), err(err) {}
    with_hastings_err(const with_hastings_err& o) : proposal_distribution(o), inner(o.inner->clone()), err(o.err) {}
    ~with_hastings_err() { delete inner; }
    double log_hastings_ratio() override { return inner->log_hastings_ratio() + err; }
    void set_chain(chain* c) override { inner->set_chain(c); }
    state draw(state& s, chain* caller) override { return inner->draw(s, caller); }
    bool is_ready() override { return inner->is_ready(); }
    proposal_distribution* clone() const override { return new with_hastings_err(*this); }
    std::string show() override { return inner->show(); }
    int type() override { return inner->type(); }
    bool support_mixing() override { return inner->support_mixing(); }
    void accept() override { inner->accept(); }
    void reject() override { inner->reject(); }
    std::string report(int style = 0) override { return inner->report(style); }
  };
  struct constant_likelihood : public gaussian_likelihood {
    explicit constant_likelihood(const stateSpace* sp) : gaussian_likelihood(std::vector<double>((size_t)sp->size() * sp->size(), 0.0), 0.0) {
      nativeSpace = *sp;
      space = &nativeSpace;
    }
  };
  static bool host_kl() {
    static const bool on = [] { const char* v = getenv("PTM_HOST_KL"); return v && *v && *v != '0'; }();   // (A/B: keep the host estimator)
    return on;
  }

 public:
  // A Gaussian in a WRAPPED dimension: the engine draws it and wraps the draw, but evaluates the plain Gaussian (it has no periodic sum,
  // the reference's wrap_probability, probability_function.cc:57-78).  The samples and the density the Metropolis-Hastings steps aim at
  // are the same distribution only while no mass reaches the seam: the target must keep seam_sigmas sigma (2e-9 of its mass beyond)
  // inside the domain on both sides.  test() refuses a target that does not, rather than report a correct proposal FAIL.
  static double seam_sigmas() { return 6.0; }
  // -1, or the first wrapped Gaussian dimension of `target` that comes nearer to its seam
  static int dimension_near_seam(const sampleable_probability_function& target) {
    std::vector<int> types;
    std::vector<double> c, h;
    const stateSpace* sp = target.get_space();
    if (!sp || !target.describe(types, c, h)) return -1;
    for (int d = 0; d < (int)types.size() && d < sp->size(); d++) {
      if (types[(size_t)d] != mixed_dist_product::gaussian || !sp->get_bound(d).isWrapped()) continue;
      double xmin, xmax;
      sp->get_bound(d).getDomainLimits(xmin, xmax);
      if (c[(size_t)d] - seam_sigmas() * h[(size_t)d] < xmin || c[(size_t)d] + seam_sigmas() * h[(size_t)d] > xmax) return d;
    }
    return -1;
  }
  proposal_tester(proposal_distribution& proposalref, sampleable_probability_function& target, bool loop = false, std::string path_ = "",
                  std::vector<int> index = std::vector<int>(), uint64_t seed = 0x5EED0001ull)
      : proposal(&proposalref), target_dist(&target), loop(loop), path(path_), seed(seed) {
    if (path != "") {   // test_proposal.hh:69-76
      if (path.back() == '/') path = path + "test_prop";
      if (index.size() > 0) path = path + "_" + std::to_string(index[0]);
      for (size_t i = 1; i < index.size(); i++) path += "-" + std::to_string(index[i]);
      std::cout << "path='" << path << "'" << std::endl;
    }
    while (index.size() > 0) {   // a set and an index: the member (and so on down the index)
      proposal_distribution_set* set = dynamic_cast<proposal_distribution_set*>(proposal);
      if (!set) break;
      proposal = set->members()[(size_t)index[0]];
      index.erase(index.begin());
    }
  }
  void write_samples(const std::vector<double>& X, int dim, const std::string& tag) const {
    if (path == "") return;
    const std::string file = path + "_" + tag + ".dat";
    std::cout << "Will write to " << file << std::endl;
    std::ofstream out(file);
    for (size_t i = 0; i * dim < X.size(); i++) out << state::from_engine(target_dist->get_space(), X.data() + i * dim, dim).get_string() << std::endl;
  }
  // test_proposal.hh:604-615: the variances, the means in out_mean
  static std::vector<double> sample_var(const std::vector<double>& X, int dim, std::vector<double>& out_mean) {
    const size_t N = X.size() / dim;
    out_mean.assign((size_t)dim, 0.0);
    for (size_t i = 0; i < N; i++) for (int j = 0; j < dim; j++) out_mean[(size_t)j] += X[i * dim + j];
    for (auto& x : out_mean) x /= N;
    std::vector<double> sum((size_t)dim, 0.0);
    for (size_t i = 0; i < N; i++)
      for (int j = 0; j < dim; j++) {
        const double diff = X[i * dim + j] - out_mean[(size_t)j];
        sum[(size_t)j] += diff * diff;
      }
    for (auto& x : sum) x /= (N - 1.0);
    return sum;
  }
  // KL_divergence(P, Q, approx_nn = false), the two searches on the device where it serves
  double kl(const std::vector<double>& P, const std::vector<double>& Q, int dim) const {
    const stateSpace* sp = target_dist->get_space();
    const long long N = (long long)(P.size() / dim), M = (long long)(Q.size() / dim);
    if (host_kl() || dim > 128) return kl_estimator::kl(P.data(), N, Q.data(), M, dim, sp).value;
    kl_estimator::check_sizes(N, M);
    std::vector<int32_t> wrapped((size_t)dim, 0);
    std::vector<double> xmin((size_t)dim, 0.0), xmax((size_t)dim, 0.0), r((size_t)N), s((size_t)N);
    for (int d = 0; sp && d < dim; d++)
      if (sp->get_bound(d).isWrapped()) { wrapped[(size_t)d] = 1; sp->get_bound(d).getDomainLimits(xmin[(size_t)d], xmax[(size_t)d]); }
    ptm_check(ptm_nn_dist2(-1, P.data(), N, P.data(), N, dim, wrapped.data(), xmin.data(), xmax.data(), 1, r.data()), "proposal_tester (ptm_nn_dist2)");
    ptm_check(ptm_nn_dist2(-1, P.data(), N, Q.data(), M, dim, wrapped.data(), xmin.data(), xmax.data(), 0, s.data()), "proposal_tester (ptm_nn_dist2)");
    return kl_estimator::combine(r, s, dim, M);
  }
  bool test(int Nsamp = 10000, double ncyc = 5, int ntry = 10, double hastings_err = 0, double min_accept = 0) {
    std::cout << "\n\nTesting proposal: " << proposal->show() << std::endl;
    std::cout << "ncyc=" << ncyc << std::endl;
    if (loop) {   // test_proposal.hh:206-225: every member of a set in turn
      proposal_distribution_set* set = dynamic_cast<proposal_distribution_set*>(proposal);
      if (set) {
        const std::vector<proposal_distribution*> members = set->members();
        const int n = (int)members.size();
        std::cout << n << " members in proposal set" << std::endl;
        for (int i = 0; i < n; i++) {
          std::cout << "Preparing and testing member " << i + 1 << " of " << n << std::endl;
          std::string subpath = path;
          if (path != "") subpath = subpath + "-" + std::to_string(i);
          std::cout << "subpath='" << subpath << "'" << std::endl;
          proposal_tester subtest(*members[(size_t)i], *target_dist, true, subpath, std::vector<int>(), seed);
          if (!subtest.test(Nsamp, ncyc, ntry, hastings_err, min_accept)) return false;
        }
        return true;
      }
    }
    if (dynamic_cast<differential_evolution*>(proposal)) {
      std::cout << "Skipping differential evolution: it draws from a chain's history, and the test has none to give it." << std::endl;
      return true;
    }
    const int dim = target_dist->getDim();
    const int near = dimension_near_seam(*target_dist);
    if (near >= 0) {
      std::cout << "The test distribution comes within " << seam_sigmas() << " sigma of the seam of wrapped dimension " << near
                << ": its samples wrap around, the density the steps aim at does not.  Not tested; move the centre inside or shrink sigma." << std::endl;
      return false;
    }
    std::unique_ptr<proposal_distribution> wrapped_prop;
    proposal_distribution* under_test = proposal;
    if (hastings_err != 0) {
      int kind = 0;
      double odf = 0;
      std::vector<double> f;
      if (device_proposal::taken_by_device(proposal) || proposal->device_describe(dim, kind, f, odf)) {
        std::cout << "hastings_err is added to the ratio on the host: it needs a host-side proposal, and this one is drawn on the device." << std::endl;
        return false;
      }
      wrapped_prop.reset(new with_hastings_err(*proposal, hastings_err));
      under_test = wrapped_prop.get();
    }
    // the test engine: one rung, Nsamp replicas, the target as the prior over a constant likelihood, no prior gate
    constant_likelihood like(target_dist->get_space());
    parallel_tempering_chains ptc(1, 1.0, 0.0, 1, false, false, -1e300);
    ptc.set_replicas(Nsamp);
    ptc.initialize(&like, target_dist, 1, seed);
    ptc.set_proposal(*under_test);
    ptm_engine* eng = ptc.engine();
    const size_t NX = (size_t)Nsamp * dim;
    std::vector<double> target_samples(NX), transformed(NX), alt_samples(NX), ll((size_t)Nsamp), lp((size_t)Nsamp);
    ptm_check(ptm_get_states(eng, target_samples.data()), "proposal_tester");
    write_samples(target_samples, dim, "target");
    int redraws = 0;   // draw 0 of every chain is the target sample, draw k > 0 the k-th redraw
    auto redraw = [&]() { ptm_check(ptm_draw_prior_rows(eng, ++redraws, 1, alt_samples.data(), ll.data(), lp.data()), "proposal_tester (redraw)"); };
    int64_t tries = 0, acc0 = 0, acc1 = 0;
    int Naccept_cum = 0, Ngoal = (int)(ncyc * Nsamp), icyc = 1, Naccept_last = 0;
    std::cout << "Applying transform:" << std::endl;
    ptm_check(ptm_get_counter_sums(eng, &tries, &acc0), "proposal_tester");
    while (Naccept_cum < Ngoal) {
      ptc.step_n(1);
      eng = ptc.engine();
      ptm_check(ptm_get_counter_sums(eng, &tries, &acc1), "proposal_tester");
      const int Naccept = (int)(acc1 - acc0);
      acc0 = acc1;
      Naccept_cum += Naccept;
      Naccept_last = Naccept;
      if (icyc % int(ncyc + 1) == 0) std::cout << 100.0 * Naccept / Nsamp << "% accepted,  " << 100.0 * Naccept_cum / Ngoal << " percent done." << std::endl;
      if (icyc == 2000 && Naccept_cum < Ngoal * 0.01) {   // not sampling fast enough: halve the goal
        ncyc = ncyc / 2.0;
        if (Naccept * 1.0 / Nsamp < min_accept) {
          std::cout << "Acceptance rate too low. Giving up." << std::endl;
          return false;
        }
        std::cout << "Sampling poorly.  Reducing to ncyc=" << ncyc << std::endl;
        Ngoal = (int)(ncyc * Nsamp);
        icyc = 0;
        Naccept_cum = 0;
      }
      icyc++;
    }
    ptm_check(ptm_get_states(eng, transformed.data()), "proposal_tester");
    write_samples(transformed, dim, "transformed");

    std::vector<double> mean, var;
    var = sample_var(target_samples, dim, mean);
    std::cout << "target mean:      "; for (auto x : mean) std::cout << x << " "; std::cout << std::endl;
    std::cout << "target var:       "; for (auto x : var) std::cout << x << " "; std::cout << std::endl;
    var = sample_var(transformed, dim, mean);
    std::cout << "transformed mean: "; for (auto x : mean) std::cout << x << " "; std::cout << std::endl;
    std::cout << "transformed var:  "; for (auto x : var) std::cout << x << " "; std::cout << std::endl;

    std::cout << "Computing KL divergences:" << std::endl;
    if (Nsamp * std::pow((double)dim, 0.7) > 4500)
      std::cout << "(exact nearest neighbours; the reference would have used approximate ones at this size)" << std::endl;
    auto fkl = [&](const std::vector<double>& P, const std::vector<double>& Q) { return kl_estimator::fake_kl(P.data(), Nsamp, Q.data(), Nsamp, dim); };
    const double KLtransformed = kl(transformed, target_samples, dim), KLtransformedX = kl(target_samples, transformed, dim);
    const double fKLtransformed = fkl(transformed, target_samples), fKLtransformedX = fkl(target_samples, transformed);
    const int fntry = 30 * ntry;
    std::vector<double> KLdiffs((size_t)ntry), fKLdiffs((size_t)fntry);
    for (int i = 0; i < ntry; i++) { redraw(); KLdiffs[(size_t)i] = kl(alt_samples, target_samples, dim); }
    std::cout << "Computing 'fake' KL divergences:" << std::endl;
    for (int i = 0; i < fntry; i++) { redraw(); fKLdiffs[(size_t)i] = fkl(alt_samples, target_samples); }
    redraw();
    const double altKLtransformed = kl(transformed, alt_samples, dim), altKLtransformedX = kl(alt_samples, transformed, dim);
    const double altfKLtransformed = fkl(transformed, alt_samples), altfKLtransformedX = fkl(alt_samples, transformed);
    last_kl.reset(new kl_verdict(KLdiffs, altKLtransformed));
    last_fkl.reset(new kl_verdict(fKLdiffs, altfKLtransformed));
    std::cout << last_kl->lines("KL", KLtransformed, KLtransformedX, altKLtransformed, altKLtransformedX, ncyc);
    std::cout << last_fkl->lines("fKL", fKLtransformed, fKLtransformedX, altfKLtransformed, altfKLtransformedX, ncyc) << std::flush;
    last_alt_fkl = altfKLtransformed;
    last_fkl_redraw_max = 0;
    for (double v : fKLdiffs) last_fkl_redraw_max = std::max(last_fkl_redraw_max, std::fabs(v));
    last_accept = Naccept_last * 1.0 / Nsamp;
    last_target = target_samples; last_transformed = transformed;
    return true;
  }
  // what the last test() found (for callers that want more than the printed lines)
  std::unique_ptr<kl_verdict> last_kl, last_fkl;
  double last_alt_fkl = 0, last_fkl_redraw_max = 0, last_accept = 0;
  std::vector<double> last_target, last_transformed;
};

class bayes_sampler : public Optioned {   // bayesian.hh:795-821
 protected:
  std::string paramfile;
  bool have_paramfile;
  void processOptions() {
    *optValue("stateFile") >> paramfile;
    if (!(paramfile == "")) have_paramfile = true;
  }

 public:
  bayes_sampler() : have_paramfile(false) {}
  virtual bayes_sampler* clone() = 0;
  virtual int initialize() = 0;
  virtual int run(const std::string& base, int ic = 0) = 0;
  virtual int analyze(const std::string& base, int ic, int Nsigma, int Nbest, bayes_likelihood& like) = 0;
  virtual bool haveParfile() { return have_paramfile; }
  virtual state getState() = 0;
  void addOptions(Options& opt, const std::string& prefix = "") override {
    Optioned::addOptions(opt, prefix);
    addOption("stateFile", "File with initialization state parameters", "");
  }
  virtual void setup(bayes_likelihood& llike, const sampleable_probability_function& prior, int output_precision = 15) = 0;
};

// ptmcmc_sampler (ptmcmc.hh:12-97, ptmcmc.cc): same calls in the same order as a reference main()
// (exampleLISA.cc:699-822):
//     ptmcmc_sampler::Init(argc, argv);  Options opt;  ptmcmc_sampler mcmc;  bayes_sampler* s0 = &mcmc;
//     s0->addOptions(opt);  like->addOptions(opt);  opt.add(Option(...));  opt.parse(argc, argv);
//     ProbabilityDist::setSeed(seed);  mcmc.setup(*like, precision);  mcmc.select_proposal();
//     for (ic...) { bayes_sampler* s = s0->clone();  s->initialize();  s->run(base, ic);  delete s; }
// select_proposal() builds the reference's default recipe (ptmcmc.cc:15-183): differential evolution + six diagonal Gaussians
// a factor gauss_step_fac apart with doubling shares (+ prior draws, + the likelihood's own proposals).  With
// --gauss_draw_frac=1 the recipe is all Gaussian and runs fused on the device; with its default (0.2) the differential-
// evolution part makes it a host-side proposal (the engine's host-proposal step).
class ptmcmc_sampler : public bayes_sampler {
  Options own_opt;   // used when the program never called addOptions (the convenience calls set() / parse() below)
  chain* cc_base;
  std::unique_ptr<parallel_tempering_chains> cc;
  proposal_distribution* cprop;
  bool have_cc, have_cprop, own_cprop;
  bayes_likelihood* chain_llike;
  const sampleable_probability_function* chain_prior;
  bool have_setup;
  int chain_Nstep, chain_Ninit, chain_nburn, output_precision;
  double swap_rate, pt_evolve_rate, pt_evolve_lpost_cut, Tmax;
  int Nstep, Nskip, Nptc, Nevery, save_every, dump_n;
  double nburn_frac;
  bool parallel_tempering;
  int istep;
  bool restarting;
  std::string restart_dir;
  int checkp_at_step;
  double ess_stop, prop_adapt_rate, dpriormin, pt_stop_evid_err = 0, rhat_stop = -1;
  int nreplicas, replica_begin = 0, device = -1;
  std::string covariance_out, quantiles_out, corner_out;
  int prop_cov_adapt_every = 0, prop_cov_adapt_rows = -1;   // every so many steps during burn-in, every rung's Gaussian factor from its own samples
  double prop_cov_adapt_scale = -1;
  std::vector<double> quantile_probs;
  int corner_bins = 20;
  double corner_range = 1.0;

  // every flag read into a typed value (a flag without a value reads as T())
  template <class T> T flag(const std::string& name) { T v = T(); *optValue(name) >> v; return v; }
  void ensure_options() { if (!haveOptions()) addOptions(own_opt); }
  void processOptions() {   // the run-shaping flags (the reference reads them in ptmcmc_sampler::processOptions, ptmcmc.cc:430-473)
    ensure_options();
    bayes_sampler::processOptions();
    checkp_at_step = flag<int>("checkp_at_step");
    restart_dir = flag<std::string>("restart_dir");
    restarting = !restart_dir.empty();
    Nevery = flag<int>("nevery");
    save_every = flag<int>("save_every");
    Nstep = flag<int>("nsteps");
    Nskip = flag<int>("nskip");
    nburn_frac = flag<double>("burn_frac");
    Nptc = flag<int>("pt");
    parallel_tempering = Nptc > 1;
    pt_evolve_rate = flag<double>("pt_evolve_rate");
    pt_evolve_lpost_cut = flag<double>("pt_evolve_lpost_cut");
    swap_rate = flag<double>("pt_swap_rate");
    Tmax = flag<double>("pt_Tmax");
    dump_n = flag<int>("pt_dump_n");
    if (dump_n < 0 || dump_n > Nptc) dump_n = Nptc;   // "0 for all" is resolved where the files are opened
    if (Nptc == 0) dump_n = 1;
    prop_adapt_rate = flag<double>("prop_adapt_rate");
    ess_stop = flag<double>("chain_ess_stop");
    rhat_stop = flag<double>("chain_rhat_stop");
    covariance_out = flag<std::string>("covariance_out");
    prop_cov_adapt_every = flag<int>("prop_cov_adapt_every");
    prop_cov_adapt_rows = flag<int>("prop_cov_adapt_rows");
    prop_cov_adapt_scale = flag<double>("prop_cov_adapt_scale");
    quantiles_out = flag<std::string>("quantiles_out");
    if (!quantiles_out.empty()) quantile_probs = parse_quantile_probs(flag<std::string>("quantile_probs"));
    corner_out = flag<std::string>("corner_out");
    if (!corner_out.empty()) {
      corner_bins = parse_corner_bins(flag<std::string>("corner_bins"));
      corner_range = parse_corner_range(flag<std::string>("corner_range"));
    }
    pt_stop_evid_err = flag<double>("pt_stop_evid_err");
    dpriormin = flag<double>("chain_dprior_min");
    nreplicas = optSet("replicas") ? flag<int>("replicas") : 1;
    replica_begin = optSet("replica_begin") ? flag<int>("replica_begin") : 0;
    device = optSet("device") ? flag<int>("device") : -1;
  }

 public:
  ptmcmc_sampler() : cc_base(nullptr), cprop(nullptr), have_cc(false), have_cprop(false), own_cprop(false), chain_llike(nullptr), chain_prior(nullptr),
                     have_setup(false), chain_Nstep(0), chain_Ninit(1), chain_nburn(0), output_precision(13), swap_rate(0.1), pt_evolve_rate(0.01),
                     pt_evolve_lpost_cut(-1), Tmax(1e9), Nstep(5000), Nskip(10), Nptc(0), Nevery(5000), save_every(1), dump_n(1), nburn_frac(0.5),
                     parallel_tempering(false), istep(0), restarting(false), checkp_at_step(-1), ess_stop(-1), prop_adapt_rate(0), dpriormin(-30), nreplicas(1) {}
  ~ptmcmc_sampler() { if (own_cprop) delete cprop; }
  // MPI start-up / shut-down in the reference (ptmcmc.cc:250-275); here the process already owns its GPU
  static void Init() { std::cout << "Running on the MI355X step engine (no MPI; ladders shard over GPUs through ptmcmc_amd.parallel)." << std::endl; }
  static void Init(int& argc, char* argv[]) { (void)argc; (void)argv; Init(); }
  static void setRNGseed(double seed) { ProbabilityDist::setSeed(seed); }
  static void Quit() { exit(0); }
  static bool static_reporting() { return true; }
  bool reporting() { return true; }

  // The sampler's flags: the NAMES and DEFAULTS are the reference's (ptmcmc.cc:375-427) -- command lines and scripts written for
  // it must parse and mean the same -- the descriptions are this build's.  "" as default: the flag has no value until given.
  // Flags of features outside this build's scope are declared too, so that such command lines parse; setup() refuses the ones
  // that would change the run (refuse_unbuilt).
  void addOptions(Options& opt, const std::string& prefix = "") override {
    bayes_sampler::addOptions(opt, prefix);
    struct decl { const char *name, *preset, *about; };
    static const char* const no_value = "<no default>";
    static const decl flags[] = {
        // run length and output
        {"nsteps", "5000", "Steps to run each chain for. [5000]"},
        {"save_every", "1", "Keep every n-th state in the chain history. [1]"},
        {"nevery", "5000", "Report and write chain-file rows every n steps. [5000]"},
        {"nskip", "10", "Of the saved states, write only every n-th to the chain files. [10]"},
        {"burn_frac", "0.5", "Leading fraction of the run treated as burn-in by the summaries. [0.5]"},
        // checkpointing
        {"checkp_at_step", "-1", "Write a checkpoint at this step and stop. [-1: never]"},
        {"checkp_at_time", "-1", "Write a checkpoint after this many hours of wall time and stop (not built here). [-1: never]"},
        {"checkp_on_sigterm_within", "0", "Look for a termination signal every n steps and checkpoint on it (not built here). [0: off]"},
        {"restart_dir", "", "Continue from the checkpoint in this directory."},
        // the temperature ladder
        {"pt", "0", "Number of temperatures of the parallel-tempering ladder. [0: no tempering]"},
        {"pt_Tmax", "1e9", "Temperature of the hottest rung. [1e9]"},
        {"pt_swap_rate", "0.10", "Exchange attempts per rung pair and step. [0.10]"},
        {"pt_evolve_rate", "0.01", "Every accepted exchange widens its temperature gap by this fraction (0: fixed ladder). [0.01]"},
        {"pt_evolve_lpost_cut", "-1", "While the ladder evolves, also widen gaps whose log-posteriors are out of order by more than this. [-1: off]"},
        {"pt_dump_n", "1", "Write chain files for the n coldest rungs (0: all of them). [1]"},
        {"pt_reboot_rate", "0", "Highest rate of restarting lagging hot chains (not built here). [0]"},
        {"pt_reboot_every", "0", "Steps between tests for lagging hot chains (not built here). [0]"},
        {"pt_reboot_grace", "0", "Steps a restarted chain is left alone (not built here). [0]"},
        {"pt_reboot_cut", "100", "Log-posterior deficit that marks a lagging chain (not built here). [100]"},
        {"pt_reboot_thermal", "0", "Temperature-dependent part of that deficit (not built here). [0]"},
        {"pt_reboot_blindly", "0", "Restart at random at this level even without a deficit (not built here). [0]"},
        {"pt_reboot_grad", no_value, "Make the grace period grow towards the cold rungs, with this mean (not built here)."},
        {"pt_stop_evid_err", "0", "Integrate the log-evidence over the ladder every 10000*(save_every/10+1) steps and stop once the standard error of the recent totals is below this. [0: off]"},
        // the default proposal recipe
        {"prop", "", "No longer used."},
        {"gauss_draw_frac", "0.20", "Share of Gaussian steps in the default proposal mixture. [0.20]"},
        {"gauss_1d_frac", "0.5", "Fraction of the Gaussian steps that move one randomly chosen parameter only. [0.5]"},
        {"gauss_step_fac", "2", "Ratio between the widths of successive Gaussian members. [2]"},
        {"gauss_temp_scaled", no_value, "Scale the Gaussian widths with the chain temperature."},
        {"prior_draw_frac", "0", "Share of independent draws from the prior in the mixture. [0]"},
        {"prior_draw_Tpow", "0", "Let the prior-draw share grow towards the hot rungs as 1 - T^-p. [0: same at every rung]"},
        {"cov_draw_frac", "0.50", "Share of Gaussian steps with the covariance of --covariance_file, if one is given. [0.50]"},
        {"covariance_file", "", "File holding a proposal covariance."},
        {"prop_adapt_rate", "0", "Rate (e.g. 1e-3) at which the Gaussian members' shares adapt to their acceptance. [0: fixed]"},
        {"prop_adapt_more", no_value, "Adapt the shares of the whole mixture, not of the Gaussian members alone."},
        {"sym_prop_frac", "0", "Share of state-space symmetry moves (not built here). [0]"},
        {"like_prop_frac", "0", "Share of the proposals the likelihood object brings along. [0]"},
        {"de_ni", "50", "Differential evolution: initial history rows per parameter. [50]"},
        {"de_eps", "1e-4", "Differential evolution: width of the small random jump. [1e-4]"},
        {"de_reduce_gamma", "4", "Differential evolution: divide the nominal jump scale by this. [4]"},
        {"de_g1_frac", "0.3", "Differential evolution: fraction of jumps made with unit scale. [0.3]"},
        {"de_mixing", no_value, "Differential evolution: draw history states from every rung of the ladder."},
        {"de_Tmix", "300", "Differential evolution: how readily other rungs' histories are used. [300]"},
        {"de_unlikely_alpha", "0", "Differential evolution: power with which improbable history states are passed over. [0: never]"},
        {"prop_test_index", "", "Index of a proposal to test in isolation (\".\": the whole proposal; a-b-c: a member of nested sets; trailing L: loop over members; each trailing +: twice the sizes)."},
        // chains
        {"chain_init_file", "", "Take the start states from this chain file instead of the prior (not built here)."},
        {"chain_ess_stop", "-1.0", "Stop as soon as the cold chain's effective sample size exceeds this. [-1: never]"},
        {"chain_ess_limit", "-1.0", "Largest effective sample size worth resolving; speeds the estimate up on long chains. [-1: none]"},
        {"chain_dprior_min", "-30", "Reject, without asking the likelihood, a proposal whose log-prior drops by more than this. [-30]"},
        // this build's additions.  Replicas: independent copies of the ladder side by side in one engine (the reference runs
        // its repeats one after the other, the caller's loop over clone() / initialize() / run()); over several GPUs one
        // process per GPU, each told which replicas of the population are its own
        {"replicas", "1", "Independent replicas of the ladder run side by side on the device (files <base>_c<w>_t<k>.dat). [1]"},
        {"replica_begin", "0", "Global index of this process's first replica (one process per GPU, disjoint ranges). [0]"},
        {"device", "-1", "GPU of this process. [-1: the current device, e.g. by HIP_VISIBLE_DEVICES]"},
        {"chain_rhat_stop", "-1.0", "Stop as soon as the split R-hat of the cold chains across the replicas, the largest over the parameters, is below this. [-1: never]"},
        {"prop_cov_adapt_every", "0", "Every so many steps while the step is below burn_frac*nsteps, replace every recorded rung's Gaussian proposal factor by one from that rung's own sampled covariance. [0: never]"},
        {"prop_cov_adapt_rows", "-1", "Saved rows of every replica that --prop_cov_adapt_every pools. [-1: the largest window every replica has, at most prop_cov_adapt_every/save_every]"},
        {"prop_cov_adapt_scale", "-1.0", "Scale of the adapted factors. [-1: 2.38/sqrt(npar)]"},
        {"covariance_out", "", "At the end of the run write the cold chains' pooled posterior mean and covariance to this file (what --covariance_file reads)."},
        {"quantiles_out", "", "At the end of the run write the cold chains' pooled posterior quantiles of every parameter to this file."},
        {"quantile_probs", "0.05,0.5,0.95", "The probabilities of --quantiles_out, separated by commas (1 to 32 values in [0, 1]). [0.05,0.5,0.95]"},
        {"corner_out", "", "At the end of the run write the cold chains' corner-plot counts -- the histogram of every parameter and of every pair of parameters -- to this file."},
        {"corner_bins", "20", "The bins of each axis of --corner_out (1 to 128). [20]"},
        {"corner_range", "1", "The share of each parameter's samples the axes of --corner_out span, centred (corner's range fraction; 1: minimum to maximum). [1]"},
    };
    for (size_t i = 0; i < sizeof flags / sizeof flags[0]; i++) addOption(flags[i].name, flags[i].about, flags[i].preset);
  }

  // ---- convenience for programs without an Options object of their own (examples/example_sampler.cc)
  void set(const std::string& name, const std::string& value) {
    ensure_options();
    std::string arg = "--" + name + "=" + value;
    std::vector<char> buf(arg.begin(), arg.end());
    buf.push_back(0);
    char* argv[2] = {nullptr, buf.data()};
    int argc = 2;
    if (own_opt.parse(argc, argv, false)) { std::cout << "ptmcmc_sampler::set: unknown option '" << name << "'" << std::endl; exit(1); }
  }
  bool parse(int argc, char* argv[]) {  // --name=value / --name; true when every flag was understood
    ensure_options();
    if (!own_opt.exists("seed")) {
      own_opt.add(Option("seed", "Seed of the random streams, a number in [0,1). [-1: the engine's fixed default key]", "-1"));
      own_opt.add(Option("outname", "Stem of the output file names. [mcmc_output]", "mcmc_output"));
      own_opt.add(Option("nchains", "Replicas of the ladder run side by side (alias of --replicas).", "1"));
    }
    int n = argc;
    const bool bad = own_opt.parse(n, argv, true);
    double seed = -1;
    std::istringstream(own_opt.value("seed")) >> seed;
    if (seed >= 0) ProbabilityDist::setSeed(seed);
    int nch = 1;
    std::istringstream(own_opt.value("nchains")) >> nch;
    if (nch > 1) set("replicas", own_opt.value("nchains"));
    return !bad;
  }
  double num(const std::string& n) { double v = 0; *optValue(n) >> v; return v; }

  // ptmcmc.cc:476-506
  void setup(int Ninit, bayes_likelihood& llike, const sampleable_probability_function& prior, proposal_distribution& prop, int output_precision_ = 15) {
    processOptions();
    chain_Nstep = Nstep; chain_Ninit = Ninit; chain_nburn = (int)(Nstep * nburn_frac); output_precision = output_precision_;
    cprop = &prop; own_cprop = false; chain_prior = &prior; chain_llike = &llike; have_setup = true; have_cprop = true;
  }
  void setup(bayes_likelihood& llike, const sampleable_probability_function& prior, int output_precision_ = 15) override {
    processOptions();
    chain_Nstep = Nstep; chain_nburn = (int)(Nstep * nburn_frac); output_precision = output_precision_;
    chain_prior = &prior; chain_llike = &llike; have_setup = true;
    refuse_unbuilt();
  }
  void setup(bayes_likelihood& llike, int output_precision_ = 15) { setup(llike, *llike.getObjectPrior(), output_precision_); }
  void refuse_unbuilt() {
    double v = 0; std::string sv;
    *optValue("pt_reboot_rate") >> v;
    if (v > 0) { std::cout << "ptmcmc_sampler: pt_reboot_rate > 0 (rebooting laggard chains) is not built in the GPU step engine." << std::endl; exit(1); }
    *optValue("chain_init_file") >> sv;
    if (!sv.empty()) { std::cout << "ptmcmc_sampler: chain_init_file is not built in the GPU step engine." << std::endl; exit(1); }
    if (Nptc < 2) { std::cout << "ptmcmc_sampler: this build drives parallel-tempering ladders: set --pt=N with N >= 2." << std::endl; exit(1); }
  }
  // a proposal of the caller's (the convenience path of examples/example_sampler.cc; the reference's deprecated setup(Ninit, ...))
  void select_proposal(proposal_distribution& p) { if (own_cprop) delete cprop; cprop = &p; own_cprop = false; have_cprop = true; }

  // ---- the default proposal (what ptmcmc_sampler::select_proposal() of the reference builds from the flags, ptmcmc.cc:15-183) -----
  // A mixture of, in this order:
  //   differential evolution   share 1 - gauss - cov - prior (not below 0): differential_evolution(snooker 0.1, de_g1_frac,
  //                            de_eps, ignore_frac 0, de_unlikely_alpha), reduce_gamma(de_reduce_gamma), optional rung mixing;
  //                            its history is seeded with de_ni initial draws per parameter
  //   prior draws              share prior_draw_frac (hot share 1, power prior_draw_Tpow), when asked for
  //   a covariance Gaussian    share cov_draw_frac, when --covariance_file names a file (read_covariance): gaussian_prop(covar,
  //                            gauss_1d_frac, gauss_temp_scaled); the reference's reader is an empty stub (ptmcmc.cc:761-764)
  //   six Gaussian steps       share gauss_draw_frac split 2 : 4 : ... : 64; widths scale_i / 100 / f with
  //                            f = (2/s)^4 s, (2/s)^4 s^2, ..., s = gauss_step_fac (2: f = 2, 4, ..., 64); each moves a single
  //                            random parameter with probability gauss_1d_frac.  With prop_adapt_rate > 0 the six form a set
  //                            of their own whose inner shares adapt.
  // and, around that, the likelihood's own proposals with share like_prop_frac.
  struct recipe {
    double gauss, gauss_1d, gauss_ratio, prior, prior_power, like_share, de_unit_frac, de_noise, de_divisor, de_mix, de_alpha, cov = 0;
    std::string cov_file;
    int de_rows_per_dim;
    bool de_mixing, adapt_all, gauss_temp_scaled;
  };
  static double unit_interval(double v) { return v < 0 ? 0.0 : (v > 1 ? 1.0 : v); }
  recipe read_recipe() {
    recipe r;
    r.prior = unit_interval(flag<double>("prior_draw_frac"));
    r.prior_power = flag<double>("prior_draw_Tpow");
    r.gauss_1d = unit_interval(flag<double>("gauss_1d_frac"));
    r.gauss = unit_interval(flag<double>("gauss_draw_frac"));
    r.gauss_ratio = std::max(1.0, flag<double>("gauss_step_fac"));
    r.like_share = flag<double>("like_prop_frac");
    r.de_rows_per_dim = flag<int>("de_ni");
    r.de_noise = flag<double>("de_eps");
    r.de_divisor = flag<double>("de_reduce_gamma");
    r.de_unit_frac = flag<double>("de_g1_frac");
    r.de_mix = flag<double>("de_Tmix");
    r.de_alpha = flag<double>("de_unlikely_alpha");
    r.de_mixing = optSet("de_mixing");
    r.adapt_all = optSet("prop_adapt_more");
    r.gauss_temp_scaled = optSet("gauss_temp_scaled");   // (without effect in the reference as well: quirk Q4)
    // the covariance Gaussian's share: none without a file (ptmcmc.cc:46-48)
    r.cov_file = flag<std::string>("covariance_file");
    r.cov = r.cov_file.empty() ? 0.0 : unit_interval(flag<double>("cov_draw_frac"));
    if (r.cov > 0) {
      if (r.prior + r.gauss + r.cov > 1) {   // ptmcmc.cc:49-53
        const double scale = r.gauss + r.cov;
        r.gauss /= scale;
        r.cov /= scale;
      }
    } else if (r.prior + r.gauss > 1) r.gauss = 1.0;   // over-subscribed: the Gaussian share is renormalised against itself
    if (flag<double>("sym_prop_frac") > 0)
      std::cout << "ptmcmc_sampler::select_proposal: state-space symmetry moves (--sym_prop_frac) are outside this build's scope; none are added." << std::endl;
    return r;
  }
  // the six Gaussian members and their relative weights 2, 4, ..., 64 (sum 126)
  void gaussian_members(const recipe& r, const std::vector<double>& scales, std::vector<proposal_distribution*>& members, std::vector<double>& weights) {
    const int count = 6;
    const double total = std::pow(2.0, count + 1) - 2;
    double divisor = std::pow(2.0 / r.gauss_ratio, 4.0), weight = 1;
    for (int k = 0; k < count; k++) {
      divisor *= r.gauss_ratio;
      weight *= 2;
      std::vector<double> sigma(scales.size());
      for (size_t i = 0; i < sigma.size(); i++) sigma[i] = scales[i] / 100.0 / divisor;
      members.push_back(new gaussian_prop(sigma, r.gauss_1d, r.gauss_temp_scaled));
      weights.push_back(weight / total);
    }
  }
  void select_proposal() {
    if (!have_setup) { std::cout << "ptmcmc_sampler::select_proposal.  Must call setup() first!" << std::endl; exit(1); }
    const recipe r = read_recipe();
    std::vector<double> scales;
    chain_llike->getScales(scales);
    const int npar = chain_prior->get_space() ? chain_prior->get_space()->size() : chain_prior->getDim();
    std::vector<proposal_distribution*> members;
    std::vector<double> cold, hot;
    double thermal_power = 0;
    // A differential-evolution member with share 0 is never picked (no uniform lies below a threshold of 0) and draws nothing:
    // leaving it out gives the same chain, and an all-Gaussian recipe can then run on the device.
    const double de_share = r.cov > 0 ? std::max(0.0, 1 - r.gauss - r.cov - r.prior) : std::max(0.0, 1 - r.gauss - r.prior);
    if (de_share > 0) {
      differential_evolution* de = new differential_evolution(0.1, r.de_unit_frac, r.de_noise, 0.0, r.de_alpha);
      de->reduce_gamma(r.de_divisor);
      if (r.de_mixing) de->support_mixing(true);
      de->mix_temperatures_more(r.de_mix);
      members.push_back(de); cold.push_back(de_share); hot.push_back(0.0);
      chain_Ninit = r.de_rows_per_dim * npar;
    } else chain_Ninit = 1;
    if (r.prior > 0) {
      members.push_back(new draw_from_dist(*chain_prior)); cold.push_back(r.prior); hot.push_back(1.0);
      thermal_power = r.prior_power;
    }
    if (!r.cov_file.empty()) {   // ptmcmc.cc:105-116: read whenever a file is named, a member when its share is above 0
      const covariance_data c = ptmgpu::read_covariance(r.cov_file, npar);
      if (r.cov > 0) { members.push_back(new gaussian_prop(c.cov, npar, r.gauss_1d, r.gauss_temp_scaled)); cold.push_back(r.cov); hot.push_back(0.0); }
    }
    std::vector<proposal_distribution*> gaussians;
    std::vector<double> gweights;
    gaussian_members(r, scales, gaussians, gweights);
    if (prop_adapt_rate > 0) {   // the Gaussian part as one member whose inner shares adapt
      members.push_back(new proposal_distribution_set(gaussians, gweights, prop_adapt_rate)); cold.push_back(r.gauss); hot.push_back(0.0);
    } else
      for (size_t k = 0; k < gaussians.size(); k++) { members.push_back(gaussians[k]); cold.push_back(gweights[k] * r.gauss); hot.push_back(0.0); }
    if (own_cprop) delete cprop;
    const double outer_rate = r.adapt_all ? prop_adapt_rate : 0.0;
    cprop = new proposal_distribution_set(members, cold, outer_rate, thermal_power, hot);
    own_cprop = true;
    std::cout << "ptmcmc_sampler::set_proposal: Tpow=" << thermal_power << ":" << std::endl;
    if (r.like_share > 0 && chain_llike->get_proposals().size() > 0) {
      std::cout << "Adding likelihood-based elements to proposal." << std::endl;
      std::vector<proposal_distribution*> theirs;
      for (auto q : chain_llike->get_proposals()) theirs.push_back(q->clone());   // (the likelihood keeps its own objects)
      std::vector<proposal_distribution*> both;
      both.push_back(cprop);
      both.push_back(new proposal_distribution_set(theirs, chain_llike->get_prop_shares(), outer_rate));
      std::vector<double> split;
      split.push_back(std::max(0.0, 1 - r.like_share));
      split.push_back(r.like_share);
      cprop = new proposal_distribution_set(both, split, prop_adapt_rate);
    }
    std::cout << "Proposal distribution is:\n" << cprop->show() << std::endl;
    have_cprop = true;
  }

  bayes_sampler* clone() override {   // ptmcmc.hh:57-76
    if (have_cc) { std::cout << "ptmcmc_sampler::clone(): Cannot clone after instantiating chain/prop." << std::endl; exit(1); }
    ptmcmc_sampler* s = new ptmcmc_sampler();
    s->copyOptioned(*this);
    if (!haveOptions()) { s->own_opt = own_opt; s->Optioned::addOptions(s->own_opt); }
    if (have_setup) s->setup(*chain_llike, *chain_prior, output_precision);
    if (have_cprop) {
      s->cprop = cprop->clone();
      s->own_cprop = true;
      s->have_cprop = true;
      s->chain_Ninit = chain_Ninit;
    }
    return s;
  }
  ptmcmc_sampler* clone_ptmcmc_sampler() { return dynamic_cast<ptmcmc_sampler*>(clone()); }
  state getState() override {
    if (!have_setup) { std::cout << "ptmcmc_sampler::getState.  Must call setup() before getState!" << std::endl; exit(1); }
    if (have_cc) return cc->getState();
    philox_random r;
    r.reseat(ProbabilityDist::engineSeed(), 0xFFFFFFFFu, 0);
    return chain_prior->drawSample(r);
  }

  // ptmcmc_sampler::checkpoint / restart (ptmcmc.cc:306-338): <path>/step_<istep>-cp/ptmcmc.cp + the ladder's own file
  void checkpoint(const std::string& path, int istep_) {
    std::ostringstream ss;
    ss << path << "/step_" << istep_ << "-cp/";
    const std::string dir = ss.str();
    std::cout << "Writing checkpoint files to dir:" << dir << std::endl;
    mkdir(dir.c_str(), 0777);
    std::ofstream os((dir + "ptmcmc.cp").c_str());
    os << istep_ << std::endl;
    cc->checkpoint(dir);
  }
  int restart(const std::string& path) {
    std::cout << "Restarting from checkpoint files in dir:" << path << std::endl;
    std::ifstream is((path + "/ptmcmc.cp").c_str());
    int istep_ = -1;
    is >> istep_;
    if (!is || istep_ < 0) { std::cout << "ptmcmc_sampler::restart: cannot read " << path << "/ptmcmc.cp" << std::endl; exit(1); }
    cc->restart(path + "/");
    return istep_;
  }

  // ---- --prop_test_index (ptmcmc.cc:185-247): test the proposal, or the member of the set a multi-index names, in isolation
  // (proposal_tester).  "." the whole proposal; "a-b-c" descends through nested sets; a trailing "L" loops over a set's members;
  // each trailing "+" doubles the sizes.  The test distribution is a Gaussian around a draw of the prior with the prior's scales,
  // halved until its +-1 sigma corners have log-prior > -100 and times 4 whenever the test gives up; in a wrapped dimension it is
  // kept 6 sigma inside the domain (below).  Nothing of the run changes:
  // the test runs on an engine of its own with a seed of its own, and no ladder seed is used up.
  int prop_test_samples = 10000, prop_test_ncyc = 500, prop_test_tries = 10;   // (the reference's sizes; a test may shrink them)
  void set_prop_test_sizes(int samples, int ncyc, int tries) { prop_test_samples = samples; prop_test_ncyc = ncyc; prop_test_tries = tries; }
  void test_prop() {
    std::string indexstring;
    *optValue("prop_test_index") >> indexstring;
    if (indexstring.length() == 0) return;
    int rigor = 0;
    while (!indexstring.empty() && indexstring.back() == '+') { rigor++; indexstring.pop_back(); }
    bool looping = false;
    if (!indexstring.empty() && indexstring.back() == 'L') { looping = true; indexstring.pop_back(); }
    std::vector<int> multiindex;
    if (indexstring != "." && !indexstring.empty()) {
      std::stringstream ss(indexstring);
      std::string elem;
      while (std::getline(ss, elem, '-')) multiindex.push_back(atoi(elem.c_str()));
      std::cout << " Testing proposal starting at multiindex:";
      for (int i : multiindex) std::cout << " " << i;
      std::cout << std::endl;
    }
    bool fits = false;
    std::vector<double> cent, sigma;
    chain_prior->getScales(sigma);
    philox_random rng;
    for (uint64_t attempt = 0; !fits; attempt++) {
      rng.reseat(ProbabilityDist::engineSeed(), 0xFFFFFFFFu, ((uint64_t)1 << 41) + attempt);   // (a stream no chain uses)
      state s0 = chain_prior->drawSample(rng);
      const int n = s0.size();
      cent = s0.get_params_vector();
      // a wrapped dimension: the test engine evaluates the plain Gaussian where the reference sums it over the periodic images
      // (wrap_probability, ptmcmc.cc:237), so the Gaussian is kept seam_sigmas sigma inside the domain -- sigma at most 1/24 of the
      // width, the centre moved in from the seam if need be (proposal_tester::dimension_near_seam)
      for (int i = 0; i < n; i++) {
        const boundary b = s0.getSpace()->get_bound(i);
        if (!b.isWrapped()) continue;
        double xmin, xmax;
        b.getDomainLimits(xmin, xmax);
        const double smax = (xmax - xmin) / (4 * proposal_tester::seam_sigmas());
        if (sigma[(size_t)i] > smax) sigma[(size_t)i] = smax;
        const double lo = xmin + proposal_tester::seam_sigmas() * sigma[(size_t)i], hi = xmax - proposal_tester::seam_sigmas() * sigma[(size_t)i];
        if (cent[(size_t)i] < lo || cent[(size_t)i] > hi) {
          std::cout << "Wrapped dimension " << i << ": centre " << cent[(size_t)i] << " moved " << proposal_tester::seam_sigmas() << " sigma in from the seam." << std::endl;
          cent[(size_t)i] = cent[(size_t)i] < lo ? lo : hi;
        }
      }
      std::vector<double> topv((size_t)n), bottomv((size_t)n);
      const double nsigcut = 1.0;
      for (int i = 0; i < n; i++) { topv[(size_t)i] = cent[(size_t)i] + sigma[(size_t)i] * nsigcut; bottomv[(size_t)i] = cent[(size_t)i] - sigma[(size_t)i] * nsigcut; }
      state top(s0.getSpace(), topv), bottom(s0.getSpace(), bottomv);
      const double logcut = -100;
      std::cout << "Checking limits: \ntop=" << top.get_string() << "\nbottom=" << bottom.get_string() << std::endl;
      if (chain_prior->evaluate_log(top) > logcut && chain_prior->evaluate_log(bottom) > logcut) fits = true;
      else for (auto& s : sigma) s /= 2;
      if (fits) {
        gaussian_dist_product dist(chain_prior->get_space(), std::valarray<double>(cent.data(), cent.size()), std::valarray<double>(sigma.data(), sigma.size()));
        std::cout << "Test distribution is: " << dist.show() << std::endl;
        const int fac = (int)std::pow(2, rigor);
        const int samples = prop_test_samples * fac, ncyc = prop_test_ncyc * fac, tries = prop_test_tries * fac;
        std::cout << "Testing on " << samples << " samples, applying proposal through " << ncyc << " cycles and calibrating with " << tries << " trials." << std::endl;
        proposal_tester testprop(*cprop, dist, looping, "./", multiindex, ProbabilityDist::engineSeed() ^ 0x7E57ull);
        fits = testprop.test(samples, ncyc, tries, 0, 0.005);
        if (!fits) for (auto& s : sigma) s *= 4;
      }
    }
  }

  int initialize() override {   // ptmcmc.cc:497-528
    if (!have_setup || !have_cprop) { std::cout << "ptmcmc_sampler::initialize.  Must call setup() and set proposal before initialization!" << std::endl; exit(1); }
    if (!parallel_tempering) { std::cout << "ptmcmc_sampler::initialize: this build drives parallel-tempering ladders: set --pt=N with N >= 2." << std::endl; exit(1); }
    int Ninit = chain_Ninit;
    if (restarting || Nstep <= 0) Ninit = 1;
    const bool do_evid = pt_stop_evid_err > 0;   // ptmcmc.cc:399,509: do_evid = verbose_evid
    cc.reset(new parallel_tempering_chains(Nptc, Tmax, swap_rate, save_every, do_evid, do_evid, dpriormin));
    cc_base = cc.get();
    have_cc = true;
    // the chain files are written from the device's history ring, every "nevery" steps: it must hold what one such
    // interval saves (up to two add_state calls per step, every save_every-th saved)
    int dn = dump_n;
    if (dn > Nptc || dn <= 0) dn = Nptc;   // ptmcmc.cc:458
    // ... and with an effective-sample-size stop (chain_ess_stop) the cold chain's whole saved history
    int kind; double odf; std::vector<double> f;
    const int dim = chain_prior->getDim();
    bool host = !cprop->device_describe(dim, kind, f, odf) && !dynamic_cast<user_gaussian_prop*>(cprop);
    if (device_proposal::taken_by_device(cprop)) host = false;   // (a device_proposal: drawn on the engine's stream, ptm_set_proposal_device)
    {
      std::vector<int> ty; std::vector<double> ce, hw;
      if (!host && !parallel_tempering_chains::prior_draws_fit_device(*cprop, chain_prior, !chain_prior->describe(ty, ce, hw))) host = true;
    }
    // A set with a differential evolution the device can draw (the default recipe): the device keeps EVERY rung's saved history of
    // the whole run -- up to two add_state calls per step, every save_every-th saved -- if that fits (16 GB here); else the host draws
    ptm_de_params deq;
    const long long de_rows = 2 + 2ll * std::max(Nevery, Nstep) / std::max(1, save_every);
    const double de_bytes = (double)de_rows * Nptc * std::max(1, nreplicas) * (8.0 * std::max(4, dim > 16 ? 32 : (dim > 8 ? 16 : (dim > 4 ? 8 : 4))) + 40.0);
    const bool de_dev = !host && cprop->device_describe_de(deq) && dim <= 128 && de_bytes < 16e9 && de_rows < (1ll << 30);
    if (!host && cprop->device_describe_de(deq) && !de_dev) host = true;
    if (de_dev) {
      if (restarting && Nstep > 0) Ninit = chain_Ninit;   // (the device's initial rows are drawn again, the same ones: they are not in the checkpoint)
      cc->keep_history((int)de_rows, Nptc);
      cc->use_device_de(true);
    } else {
      cc->keep_history(2 + 2 * ((ess_stop > 0 || rhat_stop > 0 || !covariance_out.empty() || !quantiles_out.empty() || !corner_out.empty()) ? std::max(Nevery, Nstep) : Nevery) / std::max(1, save_every), dn);
    }
    cc->set_replica_range(replica_begin, nreplicas, device);
    if (pt_evolve_rate > 0) cc->evolve_temps(pt_evolve_rate, pt_evolve_lpost_cut);   // ptmcmc.cc:512
    cc->use_host_proposals(host);
    cc->initialize(chain_llike, chain_prior, (host || de_dev) ? Ninit : 1, ProbabilityDist::nextLadderSeed());
    cc->set_proposal(*cprop);
    if (cprop->device_draw_source() || cc->draws_prior_on_device() || draw_from_dist::kept_on_host())
      std::cout << "ptmcmc_sampler::initialize: draws from the prior are made on the " << (cc->draws_prior_on_device() ? "device (ptm_set_proposal_prior_draw)" : "host (the host-proposal step)")
                << "; proposals are drawn on the " << (cc->proposals_on_host() ? "host" : "device") << std::endl;
    if (dynamic_cast<device_proposal*>(cprop))
      std::cout << "ptmcmc_sampler::initialize: the device_proposal is drawn on the " << (cc->draws_user_proposal_on_device() ? "device (ptm_set_proposal_device)" : "host (the host-proposal step)")
                << std::endl;
    test_prop();   // ptmcmc.cc:526
    return 0;
  }

  // ptmcmc_sampler::run (ptmcmc.cc:530-679): step; every "nevery" steps append what the coldest pt_dump_n chains saved
  // since the last report to <base>_t<k>.dat (k = 0 the coldest), as dumpChain writes it
  int run(const std::string& base, int ic = 0) override {
    if (!have_cc && chain_Nstep > 0) { std::cout << "ptmcmc_sampler::run.  Must call initialize() before running!" << std::endl; exit(1); }
    if (ic > 0 && restarting) { std::cout << "ptmcmc_sampler::run: Can't restart except for single chain ic=0." << std::endl; exit(1); }
    int dn = dump_n;
    if (dn > cc->multiplicity() || dn <= 0) dn = cc->multiplicity();   // ptmcmc.cc:458
    cc->limit_history_reads(dn);   // (this loop dumps rungs 0 .. dn - 1 and estimates on the cold one: no other rung's ring is read back)
    const int nrep = cc->replicas(), every = std::max(1, Nevery), skip = std::max(1, Nskip);
    std::ios_base::openmode mode = std::ios::out;
    if (ic > 0 || restarting) mode = mode | std::ios::app;   // ptmcmc.cc:538
    std::vector<std::unique_ptr<std::ofstream> > out;
    for (int w = 0; w < nrep; w++)
      for (int ich = 0; ich < dn; ich++) {   // ptmcmc.cc:547-554; replica w > 0: <base>_c<w>_t<ich>.dat
        std::ostringstream ss;
        ss << base;
        if (w + cc->replica_begin() > 0) ss << "_c" << (w + cc->replica_begin());   // (the GLOBAL replica index)
        ss << "_t" << ich << ".dat";
        out.emplace_back(new std::ofstream(ss.str().c_str(), mode));
        out.back()->precision(output_precision);
      }
    std::cout << "\nRunning chain " << ic << " for up to " << chain_Nstep << " steps." << std::endl;
    chain_llike->reset();   // ptmcmc.cc:558
    int istep0 = 0;
    if (restarting) istep0 = restart(restart_dir);   // ptmcmc.cc:564
    for (istep = istep0; istep <= chain_Nstep; istep++) {   // ptmcmc.cc:565,599-607
      if (istep == checkp_at_step) {   // ptmcmc.cc:567,593-596: write the checkpoint and stop
        std::cout << "Checkpointing triggered." << std::endl;
        checkpoint(".", istep);
        return 0;
      }
      // up to the next step somebody looks at the chains: a report / dump (every `every` steps), the checkpoint, the end
      int last = istep + (every - istep % every) % every;
      if (last > chain_Nstep) last = chain_Nstep;
      if (checkp_at_step > istep && checkp_at_step <= last) last = checkp_at_step - 1;
      if (prop_cov_adapt_every > 0) {   // ... or adapts the proposals: at multiples of prop_cov_adapt_every below the burn-in's end
        const int next = istep + (prop_cov_adapt_every - istep % prop_cov_adapt_every) % prop_cov_adapt_every;
        if (next < chain_nburn && next < last) last = next;
      }
      cc->step_n(last - istep + 1);
      istep = last;
      if (prop_cov_adapt_every > 0 && istep > 0 && 0 == istep % prop_cov_adapt_every && istep < chain_nburn) adapt_proposals();
      bool stop = false;
      if (0 == istep % every) {
        std::cout << "chain " << ic << " step " << istep << std::endl;
        std::cout << "   MaxPosterior=" << chain_llike->bestPost() << std::endl;
        for (int w = 0; w < nrep; w++)
          for (int ich = 0; ich < dn; ich++) cc->dumpChain(ich, *out[(size_t)w * dn + ich], istep - every + 1, skip, w);
        if (cc->bestEvidenceErr() < pt_stop_evid_err) {   // ptmcmc.cc:608-612
          stop = true;
          std::cout << "ptmcmc_sampler::run: Stopping based on pt_stop_evid_err criterion." << std::endl;
        }
        if (0 == istep % (every * 4)) {   // ptmcmc.cc:620-651
          std::cout << "Proposal report:\n" << cc->report_prop(1) << "\nacceptance report:\n" << cc->report_prop(0) << std::endl;
          if (ess_stop > 0) {   // ptmcmc.cc:628-649
            double esslimit = -1;
            *optValue("chain_ess_limit") >> esslimit;
            std::cout << "Effective sample size test" << std::endl;
            // a population on the device: one estimate of every replica; replica 0's is the reference's line and the criterion
            // (the reference's behaviour), the population's spread follows it
            std::pair<double, int> ess_len;
            if (nrep > 1 && cc->ess_on_device_possible()) {
              const std::vector<std::pair<double, int> > all = cc->report_effective_samples_all(-1, save_every * 1000, save_every, esslimit);
              ess_len = all[0];
              cc->print_effective_samples(-1, ess_len);
              std::vector<double> e;
              for (size_t k = 0; k < all.size(); k++) e.push_back(all[k].first);
              std::sort(e.begin(), e.end());
              std::cout << "Over " << e.size() << " replicas: ess min=" << e.front() << " median=" << e[e.size() / 2] << " max=" << e.back() << std::endl;
            } else ess_len = cc->report_effective_samples(-1, save_every * 1000, save_every, esslimit);
            if (ess_len.first > ess_stop) {
              stop = true;
              std::cout << "ptmcmc_sampler::run: Stopping based on chain_ess_stop Effective Sample Size criterion." << std::endl;
            }
          }
          if (rhat_stop > 0) {   // this build's own: do the replicas' cold chains agree?  (the reference runs one ladder)
            // the newest (1 - burn_frac) share of the saved rows every replica has, an even count
            int nrows = (int)((1.0 - nburn_frac) * cc->rhat_rows_available(0));
            nrows -= nrows % 2;
            if (nrows >= 4) {
              const rhat_estimator::result r = cc->split_rhat(0, -1, nrows);
              const int k = r.worst();
              char line[160];
              snprintf(line, sizeof line, "Split R-hat over %d replicas, %d rows: max=%.17g (par %d)", nrep, nrows, r.rhat[(size_t)k], k);
              std::cout << line << std::endl;
              if (r.rhat[(size_t)k] < rhat_stop) {   // (a NaN is below nothing)
                stop = true;
                std::cout << "ptmcmc_sampler::run: Stopping based on chain_rhat_stop criterion." << std::endl;
              }
            }
          }
        }
      }
      if (stop) break;
    }
    for (size_t k = 0; k < out.size(); k++) *out[k] << "\n" << std::endl;   // ptmcmc.cc:665
    if (!covariance_out.empty()) write_covariance(covariance_out);
    if (!quantiles_out.empty()) write_quantiles(quantiles_out);
    if (!corner_out.empty()) write_corner(corner_out);
    std::cout << "Finished running chain " << ic << "." << std::endl;
    return 0;
  }
  // --prop_cov_adapt_every: every recorded rung's Gaussian factor from the rows saved since the last adaptation (or as many as
  // --prop_cov_adapt_rows says), of every replica.  Only during burn-in: the rows the summaries keep come from fixed proposals.
  void adapt_proposals() {
    int rows = prop_cov_adapt_rows;
    if (rows < 1) {
      rows = prop_cov_adapt_every / std::max(1, save_every);
      for (int r = 0; r < cc->history_rungs(); r++) rows = std::min(rows, cc->rhat_rows_available(r));
    }
    if (rows < 1 || (long long)rows * cc->replicas() < 2) return;   // (nothing saved yet to adapt to)
    const parallel_tempering_chains::proposal_adapt_result r = cc->adapt_gaussian_proposals(rows, prop_cov_adapt_scale);
    if (r.rungs <= 0) return;
    std::cout << "Proposal factors from " << r.rows << " rows x " << cc->replicas() << " replicas: " << r.set << " of " << r.rungs << " rungs set, " << r.not_finite
              << " kept (not finite), " << r.not_positive << " kept (not positive definite)" << (cc->proposal_adapt_ran_on_device() ? " (device)" : " (host)") << " at step " << istep << std::endl;
  }
  // ptmcmc_sampler::write_covariance / read_covariance (ptmcmc.cc:761-768, empty there).  The cold rung's pooled moments over the
  // newest (1 - burn_frac) share of the saved rows every replica has, in the format read_covariance reads.
  void write_covariance(const std::string& file) {
    const int nrep = cc->replicas();
    int nrows = (int)((1.0 - nburn_frac) * cc->rhat_rows_available(0));
    if (nrows < 1 || (long long)nrep * nrows < 2) { std::cout << "ptmcmc_sampler::write_covariance: too few saved rows (" << nrows << " of " << nrep << " replicas); '" << file << "' is not written." << std::endl; return; }
    const int npar = chain_prior->getDim();
    if (npar > 128) { std::cout << "ptmcmc_sampler::write_covariance: a covariance is estimated for up to 128 parameters; '" << file << "' is not written." << std::endl; return; }
    const moments_estimator::result r = cc->posterior_moments(0, -1, nrows);
    std::vector<std::string> names;
    for (int i = 0; i < npar; i++) names.push_back(chain_prior->get_space() ? chain_prior->get_space()->get_name(i) : std::string("[unnamed]"));
    ptmgpu::write_covariance(file, r.mean, r.cov, r.count, nrep, nrows, names);
    double smin = 0, smax = 0;
    for (int i = 0; i < npar; i++) {
      const double sd = std::sqrt(r.var[(size_t)i]);
      if (!i || sd < smin) smin = sd;
      if (!i || sd > smax) smax = sd;
    }
    std::cout << "Posterior moments over " << nrep << " replicas, " << nrows << " rows: " << npar << " parameters, standard deviations " << smin << " .. " << smax
              << (cc->moments_ran_on_device() ? " (device)" : " (host)") << ", written to " << file << std::endl;
  }
  covariance_data read_covariance(const std::string& file) { return ptmgpu::read_covariance(file, chain_prior->getDim()); }
  // --quantile_probs: numbers separated by commas; refuses, with a message and exit(1), an empty list, more than 32 values, a value
  // that is not a number or lies outside [0, 1]
  static std::vector<double> parse_quantile_probs(const std::string& text) {
    auto refuse = [&](const std::string& why) { std::cout << "ptmcmc_sampler: --quantile_probs='" << text << "': " << why << std::endl; exit(1); };
    std::vector<double> probs;
    size_t at = 0;
    while (at <= text.size()) {
      const size_t comma = std::min(text.find(',', at), text.size());
      const std::string word = text.substr(at, comma - at);
      char* end = nullptr;
      const double p = strtod(word.c_str(), &end);
      if (word.empty() || end == word.c_str() || *end) refuse("not a number: '" + word + "'");
      if (!(p >= 0.0 && p <= 1.0)) refuse("a probability is outside [0, 1]");
      probs.push_back(p);
      at = comma + 1;
    }
    if (probs.size() > 32) refuse("at most 32 probabilities");
    return probs;
  }
  // The cold rung's pooled quantiles over the newest (1 - burn_frac) share of the saved rows every replica has, in the format
  // read_quantiles reads.
  void write_quantiles(const std::string& file) {
    const int nrep = cc->replicas();
    const int nrows = (int)((1.0 - nburn_frac) * cc->rhat_rows_available(0));
    if (nrows < 1) { std::cout << "ptmcmc_sampler::write_quantiles: too few saved rows (" << nrows << " of " << nrep << " replicas); '" << file << "' is not written." << std::endl; return; }
    const int npar = chain_prior->getDim();
    const quantile_estimator::result r = cc->posterior_quantiles(quantile_probs, 0, -1, nrows);
    std::vector<std::string> names;
    for (int i = 0; i < npar; i++) names.push_back(chain_prior->get_space() ? chain_prior->get_space()->get_name(i) : std::string("[unnamed]"));
    ptmgpu::write_quantiles(file, r, nrep, nrows, names);
    std::cout << "Posterior quantiles over " << nrep << " replicas, " << nrows << " rows: " << npar << " parameters at " << quantile_probs.size() << " probabilities"
              << (cc->quantiles_ran_on_device() ? " (device)" : " (host)") << ", written to " << file << std::endl;
  }
  // --corner_bins: a whole number in 1..128; --corner_range: a number in (0, 1].  Refused with a message and exit(1) otherwise
  static int parse_corner_bins(const std::string& text) {
    char* end = nullptr;
    const long n = strtol(text.c_str(), &end, 10);
    if (text.empty() || end == text.c_str() || *end || n < 1 || n > 128) { std::cout << "ptmcmc_sampler: --corner_bins='" << text << "': a whole number in 1..128 is needed" << std::endl; exit(1); }
    return (int)n;
  }
  static double parse_corner_range(const std::string& text) {
    char* end = nullptr;
    const double c = strtod(text.c_str(), &end);
    if (text.empty() || end == text.c_str() || *end || !(c > 0.0 && c <= 1.0)) { std::cout << "ptmcmc_sampler: --corner_range='" << text << "': a number in (0, 1] is needed" << std::endl; exit(1); }
    return c;
  }
  // the probabilities whose quantiles are the ends of an axis that spans the share c of the samples: 0 and 1 for c = 1
  static std::vector<double> corner_probs(double c) { return c >= 1.0 ? std::vector<double>{0.0, 1.0} : std::vector<double>{(1.0 - c) / 2.0, (1.0 + c) / 2.0}; }
  // a parameter whose two ends are equal gets lo - 0.5, hi + 0.5 (numpy's rule for an empty range)
  static void widen_equal_range(double& lo, double& hi) {
    if (lo == hi) { lo -= 0.5; hi += 0.5; }
  }
  // The cold rung's corner-plot counts over the newest (1 - burn_frac) share of the saved rows every replica has, the axes from
  // the sample's own quantiles, in the format read_corner reads.
  void write_corner(const std::string& file) {
    const int nrep = cc->replicas();
    const int nrows = (int)((1.0 - nburn_frac) * cc->rhat_rows_available(0));
    if (nrows < 1) { std::cout << "ptmcmc_sampler::write_corner: too few saved rows (" << nrows << " of " << nrep << " replicas); '" << file << "' is not written." << std::endl; return; }
    const int npar = chain_prior->getDim();
    const quantile_estimator::result q = cc->posterior_quantiles(corner_probs(corner_range), 0, -1, nrows);
    std::vector<double> lo((size_t)npar), hi((size_t)npar);
    for (int i = 0; i < npar; i++) {
      lo[(size_t)i] = q.q[(size_t)i];
      hi[(size_t)i] = q.q[(size_t)npar + i];
      widen_equal_range(lo[(size_t)i], hi[(size_t)i]);
    }
    const histogram_estimator::result r = cc->posterior_histograms(lo, hi, corner_bins, 0, -1, nrows, true);
    std::vector<std::string> names;
    for (int i = 0; i < npar; i++) names.push_back(chain_prior->get_space() ? chain_prior->get_space()->get_name(i) : std::string("[unnamed]"));
    ptmgpu::write_corner(file, r, nrep, nrows, names);
    std::cout << "Posterior histograms over " << nrep << " replicas, " << nrows << " rows: " << npar << " parameters, " << histogram_estimator::npairs(npar) << " pairs, " << corner_bins << " bins"
              << (cc->histograms_ran_on_device() ? " (device)" : " (host)") << ", written to " << file << std::endl;
  }
  // ptmcmc_sampler::analyze (ptmcmc.cc:681-755): the 1-sigma sample files of the reference need bayes_likelihood::write /
  // writeFine (signal / data modelling, out of this build's scope); what remains is its summary line
  int analyze(const std::string& base, int ic, int Nsigma, int Nbest, bayes_likelihood& like) override {
    (void)base; (void)Nsigma; (void)Nbest; (void)like;
    if (!have_cc) { std::cout << "ptmcmc_sampler::analyze.  Must call initialize() before analyze()!" << std::endl; exit(1); }
    std::cout << "chain " << ic << ": best_post " << chain_llike->bestPost() << ", state=" << chain_llike->bestState().get_string() << std::endl;
    return 0;
  }
  parallel_tempering_chains* chains() { return cc.get(); }
  proposal_distribution* selected_proposal() { return have_cprop ? cprop : nullptr; }   // what select_proposal chose or built
};

}  // namespace ptmgpu
#endif
