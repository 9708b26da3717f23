"""The device-prior plug-in (ptm_set_prior_device) without a GPU: its entry point and typedef are declared, exported and bound, it
checks its arguments before any device is touched, the library holds its kernels, the prior gate -- the one function the host-prior
path and the device kernel share -- holds against a literal restatement of the rule (a stand-alone program under the sanitizers), and
the C++ facade's device_prior compiles as C++11 without HIP headers."""
import ctypes as C
import os
import re
import subprocess
import tempfile

from ptmcmc_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ptmcmc_amd", "csrc")


def test_entry_point_is_declared_exported_and_bound():
    lib = C.CDLL(E.LIB_PATH)
    txt = open(os.path.join(ROOT, "include", "ptm_engine.h")).read()
    assert re.search(r"typedef void \(\*ptm_logprior_device_fn\)\(void\* user, void\* stream, int n_rows, int dim, const double\* X_dev, "
                     r"const int32_t\* count_dev,\s+double\* out_lprior_dev\);", txt)
    assert "int ptm_set_prior_device(ptm_engine* e, ptm_logprior_device_fn fn, void* user);" in txt
    assert "ptm_set_prior_device" in E.EXPORTS and hasattr(lib, "ptm_set_prior_device")
    assert lib.ptm_abi_version() == 3      # an addition: the version stays
    for m in ("set_prior_device", "set_prior_device_c"):
        assert callable(getattr(E.Engine, m, None)), m
    assert "ENQUEUE" in E.Engine.set_prior_device.__doc__


def test_arguments_are_checked_before_the_device_is_used():
    L = E.load()
    cb = E.LOGLIKE_DEVICE_FN(lambda *a: None)
    assert L.ptm_set_prior_device(None, C.cast(cb, C.c_void_p), None) == -1
    assert b"null" in L.ptm_last_error()
    assert L.ptm_set_prior_device(None, None, None) == -1


def test_the_library_holds_the_kernels_and_the_host_path_shares_the_gate():
    blob = open(E.LIB_PATH, "rb").read()
    for name in (b"devprior_gate_kernel", b"devprior_valid_kernel", b"devprior_states_kernel"):
        assert name in blob, name
    eng = open(os.path.join(CSRC, "ptm_engine.hip")).read()
    host = eng[eng.index("static int callback_host_part("):eng.index("// ---- device likelihood (ptm_set_target_device)")]
    assert "prior_gate(" in host and "-1e200" not in host      # the rule lives in the header alone
    hdr = open(os.path.join(CSRC, "ptm_devprior_kernels.hpp")).read()
    assert hdr.count("-1e200") >= 1 and "prior_gate(nl, lp[c], ll[c], b, min_prior)" in hdr


def test_prior_gate_against_the_rule_under_the_sanitizers():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "devprior_gate")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "cxx", "devprior_gate_main.cc"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"checks=(\d+)\n", r.stdout)
    assert m and int(m.group(1)) >= 2 * 7 * 3 * 6 * 2, r.stdout


def test_a_device_prior_subclass_compiles_against_the_facade_as_cxx11():
    src = r'''
#include "ptmcmc_gpu.hh"
using namespace ptmgpu;
struct my_prior : public device_prior {
  mutable int calls = 0;
  my_prior(const stateSpace* sp) : device_prior(sp) { dim = 2; }
  void evaluate_log_prior_device(void* stream, int n_rows, int dim, const double* X_dev, const int32_t* count_dev, double* out_dev) const override {
    (void)stream; (void)n_rows; (void)dim; (void)X_dev; (void)count_dev; (void)out_dev; calls++;
  }
  double evaluate_log(state& s) const override { return -0.5 * s.get_param(0) * s.get_param(0); }
  state drawSample(Random& rng) const override { std::valarray<double> x(2); x[0] = rng.Next(); x[1] = rng.Next(); return state(get_space(), x); }
};
int main() {
  stateSpace sp(2);
  my_prior p(&sp);
  ptm_logprior_device_fn f = &device_prior::device_trampoline;
  f((void*)static_cast<const device_prior*>(&p), nullptr, 0, 2, nullptr, nullptr, nullptr);
  std::vector<int> t;
  std::vector<double> c, h;
  const sampleable_probability_function* q = &p;
  return (p.calls == 1 && !q->describe(t, c, h) && dynamic_cast<const device_prior*>(q) != nullptr) ? 0 : 1;
}
'''
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "t.cc")
        open(p, "w").write(src)
        r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                            "-I", os.path.join(ROOT, "ptmcmc_amd", "host"), p], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
