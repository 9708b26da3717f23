"""The device-proposal plug-in (ptm_set_proposal_device) without a GPU: its entry point and typedefs are declared, exported and
bound, it checks its arguments before any device is touched, the build holds its kernels for every padded dimension, and the
C++ facade's device_proposal compiles as C++11 without HIP headers."""
import ctypes as C
import os
import subprocess
import tempfile

from ptmcmc_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_exported_and_bound():
    lib = C.CDLL(E.LIB_PATH)
    txt = open(os.path.join(ROOT, "include", "ptm_engine.h")).read()
    assert "typedef void (*ptm_propose_device_fn)(" in txt
    assert "typedef void (*ptm_proposal_result_device_fn)(" in txt
    assert "int ptm_set_proposal_device(ptm_engine* e, ptm_propose_device_fn propose, ptm_proposal_result_device_fn result, void* user);" in txt
    assert "ptm_set_proposal_device" in E.EXPORTS and hasattr(lib, "ptm_set_proposal_device")
    assert lib.ptm_abi_version() == 3      # an addition: the version stays
    for m in ("set_proposal_device", "set_proposal_device_c"):
        assert callable(getattr(E.Engine, m, None)), m
    assert "ENQUEUE" in E.Engine.set_proposal_device.__doc__


def test_arguments_are_checked_before_the_device_is_used():
    L = E.load()
    cb = E.PROPOSE_DEVICE_FN(lambda *a: None)
    rcb = E.PROPOSAL_RESULT_DEVICE_FN(lambda *a: None)
    assert L.ptm_set_proposal_device(None, C.cast(cb, C.c_void_p), C.cast(rcb, C.c_void_p), None) == -1
    assert b"null" in L.ptm_last_error()
    assert L.ptm_set_proposal_device(None, None, None, None) == -1


def test_the_library_holds_the_kernels_for_every_padded_dimension():
    blob = open(E.LIB_PATH, "rb").read()
    for name in (b"devprop_ids_kernel", b"devprop_result_kernel"):
        assert name in blob, name
    for dp in (4, 8, 16, 32, 64, 128, 256, 512, 1024):
        assert b"devprop_unpack_kernelILi%dEE" % dp in blob, dp      # (the mangled instantiation)


def test_a_device_proposal_subclass_compiles_against_the_facade_as_cxx11():
    src = r'''
#include "ptmcmc_gpu.hh"
using namespace ptmgpu;
struct my_prop : public device_proposal {
  int calls = 0, results = 0;
  void draw_device(void* stream, int n_rows, int dim, const double* X_cur_dev, const int32_t* rung_dev, const int32_t* walker_dev,
                   const int32_t* count_dev, uint64_t step, double* X_prop_dev, double* log_hastings_dev, int32_t* type_dev,
                   int32_t* valid_dev) override {
    (void)stream; (void)n_rows; (void)dim; (void)X_cur_dev; (void)rung_dev; (void)walker_dev; (void)count_dev; (void)step;
    (void)X_prop_dev; (void)log_hastings_dev; (void)type_dev; (void)valid_dev; calls++;
  }
  bool has_result_device() const override { return true; }
  void result_device(void*, int, const int32_t*, const int32_t*, const int32_t*, const int32_t*) override { results++; }
  state draw(state& s, chain* caller) override { (void)caller; log_hastings = 0; return s; }
  proposal_distribution* clone() const override { return new my_prop(*this); }
};
int main() {
  my_prop p;
  ptm_propose_device_fn f = &device_proposal::device_trampoline;
  ptm_proposal_result_device_fn g = &device_proposal::device_result_trampoline;
  (void)f; (void)g;
  proposal_distribution* q = p.clone();
  const bool dev = device_proposal::taken_by_device(q);
  delete q;
  return dev ? 0 : 1;
}
'''
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "t.cc")
        open(p, "w").write(src)
        r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                            "-I", os.path.join(ROOT, "ptmcmc_amd", "host"), p], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
