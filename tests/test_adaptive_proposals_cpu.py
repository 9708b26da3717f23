"""The adaptive proposal set (ptm_set_proposal_adaptive) without a GPU: its entry points are declared, exported and bound, refuse NULL
and invalid arguments before any device is used, have no CPU fallback -- and tests/adaptive_model.py, the restatement the GPU tests
check the engine against, follows the C++ facade's proposal_distribution_set outcome by outcome."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import adaptive_model as AM
from ptmcmc_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptm_set_proposal_adaptive", "ptm_get_proposal_adapt_state", "ptm_set_proposal_adapt_state")


def test_new_entry_points_are_declared_exported_and_bound():
    lib = C.CDLL(E.LIB_PATH)
    txt = open(os.path.join(ROOT, "include", "ptm_engine.h")).read()
    assert "typedef struct ptm_adaptive_set {" in txt
    for name in NEW:
        assert name in E.EXPORTS and hasattr(lib, name) and (name + "(") in txt, name
    assert lib.ptm_abi_version() == 3
    for m in ("set_proposal_adaptive", "proposal_adapt_state", "set_proposal_adapt_state"):
        assert hasattr(E.Engine, m), m


def test_null_arguments_are_refused_before_the_device_is_used():
    L = E.load()
    a = E.PtmAdaptiveSet(2, -1, 0, 0.1, 0.0)
    d = (C.c_double * 16)()
    i = (C.c_int32 * 16)()
    dp = C.cast(d, E._dp)
    ip = C.cast(i, E._i32p)
    assert L.ptm_set_proposal_adaptive(None, C.byref(a), dp, dp, dp, dp, ip, ip) == -1
    assert b"null" in L.ptm_last_error()
    assert L.ptm_set_proposal_adaptive(None, None, dp, dp, dp, dp, ip, ip) == -1
    assert L.ptm_get_proposal_adapt_state(None, dp, dp, ip, ip) == -1
    assert b"null" in L.ptm_last_error()
    assert L.ptm_set_proposal_adapt_state(None, dp, dp, ip, ip) == -1


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present")
def test_no_cpu_fallback_for_adaptive_sets():
    assert E.device_count() == 0
    with pytest.raises(E.PtmError) as ei:
        E.Engine(6, 20, 1)
    assert "no gfx950" in str(ei.value)


_PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ptmcmc_gpu.hh"
using namespace ptmgpu;
// uniforms read from stdin, one per Next()
struct scripted : public Random {
  double Next() override { double u; if (scanf("%lf", &u) != 1) exit(3); return u; }
};
struct toy_chain : public chain {
  std::shared_ptr<Random> rng = std::make_shared<scripted>();
  void step() override {}
  state getState(int, bool) override { return state(); }
  double getLogPost(int, bool) override { return 0; }
  double getLogLike(int, bool) override { return 0; }
  int getStep() override { return 0; }
  std::shared_ptr<Random> getPRNG() override { return rng; }
};
static void dump(proposal_distribution_set& s) {
  std::vector<double> w, th;
  std::vector<int> bits, cnt;
  s.adapt_state(w, th, bits, cnt);
  for (double v : w) printf("%a ", v);
  for (double v : th) printf("%a ", v);
  printf("%d %d %d %d\n", bits[0], bits[1], cnt[0], cnt[1]);
}
int main(int argc, char** argv) {
  const int K = atoi(argv[1]), nested = atoi(argv[2]), Ki = atoi(argv[3]), steps = atoi(argv[5]);
  const double rate = atof(argv[4]), rate_in = atof(argv[6]);
  std::vector<proposal_distribution*> top, inner;
  std::vector<double> ts, is;
  for (int k = 0; k < Ki; k++) { inner.push_back(new proposal_distribution()); is.push_back(2.0 * (k + 1)); }
  for (int k = 0; k < K; k++) {
    if (k == nested) top.push_back(new proposal_distribution_set(inner, is, rate_in));
    else top.push_back(new proposal_distribution());
    ts.push_back(1.0 + k);
  }
  proposal_distribution_set s(top, ts, rate);
  toy_chain ch;
  state st;
  dump(s);
  for (int n = 0; n < steps; n++) {
    s.draw(st, &ch);
    int acc;
    if (scanf("%d", &acc) != 1) return 4;
    if (acc) s.accept(); else s.reject();
    dump(s);
  }
  return 0;
}
'''


@pytest.mark.parametrize("K,nested,Ki,rate,rate_in", [(3, -1, 0, 0.3, 0.0), (6, -1, 0, 0.01, 0.0), (2, 1, 6, 0.0, 0.3), (3, 0, 4, 0.2, 0.3),
                                                      (2, 1, 6, 0.01, 0.01)])
def test_the_model_follows_the_facade_outcome_by_outcome(K, nested, Ki, rate, rate_in):
    """scripted uniforms and outcomes into the facade's proposal_distribution_set and into adaptive_model.ChainSet: the same picks,
    and the same shares and thresholds -- every bit -- after every outcome"""
    steps = 400
    rng = np.random.default_rng(K * 10 + Ki)
    top = [1.0 + k for k in range(K)]
    inner = [2.0 * (k + 1) for k in range(Ki)] if nested >= 0 else None
    cs = AM.ChainSet(top, rate, nested, inner, rate_in)
    script, want = [], []

    def row():
        w, th, bits, cnt = cs.state()
        return " ".join(float(v).hex() for v in w + th) + " %d %d %d %d" % tuple(bits + cnt)

    want.append(row())
    for _ in range(steps):
        xt = float(rng.uniform()) if K > 1 else 0.0
        xi = float(rng.uniform())
        acc = int(rng.uniform() < 0.4)
        i, j, _ = cs.pick(xt, xi)
        script += (["%r" % xt] if K > 1 else []) + (["%r" % xi] if j >= 0 and Ki > 1 else []) + [str(acc)]
        cs.outcome(i, j, acc)
        want.append(row())
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.cc"), os.path.join(d, "t")
        open(src, "w").write(_PROGRAM)
        r = subprocess.run(["g++", "-std=c++11", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ptmcmc_amd", "host"),
                            src, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        out = subprocess.run([exe, str(K), str(nested), str(Ki), repr(rate), str(steps), repr(rate_in)], input=" ".join(script), capture_output=True,
                             text=True, timeout=60)
        assert out.returncode == 0, out.stderr
    got = out.stdout.split("\n")[:steps + 1]

    def norm(line):   # %a prints 0x1.8p-1 style; Python's hex() 0x1.8000000000000p-1: compare the values
        parts = line.split()
        n = 2 * (K + (Ki if nested >= 0 else 0))
        return [float.fromhex(p) for p in parts[:n]] + [int(p) for p in parts[n:]]
    for k, (g, w) in enumerate(zip(got, want)):
        assert norm(g) == norm(w), (k, g, w)
