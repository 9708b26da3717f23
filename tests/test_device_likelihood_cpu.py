"""The device-likelihood plug-in (ptm_set_target_device) without a GPU: its entry points exist, refuse NULL arguments before any
device is touched, and have no CPU fallback; the C++ facade's device_likelihood compiles as C++11 without HIP headers."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from ptmcmc_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptm_set_target_device", "ptm_target_device_rows", "ptm_get_best_evaluated")


def test_new_entry_points_are_declared_exported_and_bound():
    lib = C.CDLL(E.LIB_PATH)
    txt = open(os.path.join(ROOT, "include", "ptm_engine.h")).read()
    assert "typedef void (*ptm_loglike_device_fn)(" in txt
    for name in NEW:
        assert name in E.EXPORTS and hasattr(lib, name) and (name + "(") in txt, name
    assert lib.ptm_abi_version() == 3


def test_null_arguments_are_refused_before_the_device_is_used():
    L = E.load()
    cb = E.LOGLIKE_DEVICE_FN(lambda *a: None)
    fp = C.cast(cb, C.c_void_p)
    assert L.ptm_set_target_device(None, fp, None, None, None) == -1
    assert b"null" in L.ptm_last_error()
    assert L.ptm_set_target_device(None, None, None, None, None) == -1
    assert L.ptm_target_device_rows(None) == -1
    lp = C.c_double()
    x = (C.c_double * 4)()
    assert L.ptm_get_best_evaluated(None, C.byref(lp), x) == -1
    assert b"null" in L.ptm_last_error()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present")
def test_no_cpu_fallback_for_a_device_likelihood():
    assert E.device_count() == 0
    with pytest.raises(E.PtmError) as ei:
        E.Engine(6, 20, 1)
    assert "no gfx950" in str(ei.value)
    # the binding's methods exist, and there is no engine to hand them to
    for m in ("set_target_device", "set_target_device_c", "best_evaluated", "target_device_rows"):
        assert hasattr(E.Engine, m), m


def test_a_device_likelihood_subclass_compiles_against_the_facade_as_cxx11():
    src = r'''
#include "ptmcmc_gpu.hh"
using namespace ptmgpu;
struct my_like : public device_likelihood {
  int calls = 0;
  void evaluate_log_device(void* stream, int n_rows, int dim, const double* X_dev, const int32_t* count_dev, double* out_dev) override {
    (void)stream; (void)n_rows; (void)dim; (void)X_dev; (void)count_dev; (void)out_dev; calls++;
  }
};
int main() {
  my_like l;
  ptm_loglike_device_fn f = &device_likelihood::device_trampoline;
  (void)f;
  state s = l.bestState();
  (void)s;
  return l.bestPost() > 0 ? 1 : 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "t.cc")
        open(p, "w").write(src)
        r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                            "-I", os.path.join(ROOT, "ptmcmc_amd", "host"), p], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
