"""Draws from the prior as a device member of the proposal set (ptm_set_proposal_prior_draw) without a GPU: the entry point is declared,
exported and bound; and the facade's sampler recipe with --prior_draw_frac --prior_draw_Tpow describes itself to the device rung by
rung -- cumulative shares bit for bit those of tests/prior_draw_model.py's thermal reset_bins, the prior member's index reported --
while the same recipe with an adapting top set (--prop_adapt_more) declines."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

import prior_draw_model as PM
from ptmcmc_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_is_declared_exported_and_bound():
    lib = C.CDLL(E.LIB_PATH)
    txt = open(os.path.join(ROOT, "include", "ptm_engine.h")).read()
    name = "ptm_set_proposal_prior_draw"
    assert name in E.EXPORTS and hasattr(lib, name) and ("int " + name + "(ptm_engine* e, int member);") in txt
    assert lib.ptm_abi_version() == 3
    assert hasattr(E.Engine, "set_proposal_prior_draw")
    L = E.load()
    assert L.ptm_set_proposal_prior_draw(None, 0) == -1 and b"null" in L.ptm_last_error()


_PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "ptmcmc_gpu.hh"
using namespace ptmgpu;
struct rung : public chain {   // a chain that only knows its temperature
  double beta;
  explicit rung(double b) : beta(b) {}
  void step() override {}
  state getState(int, bool) override { return state(); }
  double getLogPost(int, bool) override { return 0; }
  double getLogLike(int, bool) override { return 0; }
  int getStep() override { return 0; }
  int getDim() override { return 3; }
  double invTemp() override { return beta; }
};
int main(int argc, char** argv) {
  const int D = 3, Nt = 5;
  stateSpace space(D);
  std::vector<std::string> names = {"a", "b", "c"};
  space.set_names(names);
  std::vector<double> P = {2.0, 0.6, 0.0, 0.6, 1.0, -0.3, 0.0, -0.3, 1.5};
  gaussian_likelihood like(P, 0.0);
  std::vector<std::string> types(D, "uni");
  std::vector<double> centers(D, 0.0), scales(D, 4.0);
  like.basic_setup(&space, types, centers, scales);
  ptmcmc_sampler mcmc;
  mcmc.set("pt", "5"); mcmc.set("pt_Tmax", "100");
  if (!mcmc.parse(argc, argv)) { printf("bad option\n"); return 2; }
  mcmc.setup(like);
  mcmc.select_proposal();
  proposal_distribution* prop = mcmc.selected_proposal();
  proposal_distribution_set* set = dynamic_cast<proposal_distribution_set*>(prop);
  int kind; double odf; std::vector<double> f;
  const bool dev = prop->device_describe(D, kind, f, odf);
  printf("device %d prior_member %d fits %d\n", dev ? 1 : 0, set ? set->device_prior_member() : -9,
         parallel_tempering_chains::prior_draws_fit_device(*prop, like.getObjectPrior().get(), false) ? 1 : 0);
  if (!dev) return 0;
  const double tratio = std::exp(std::log(100.0) / (Nt - 1));   // the ladder parallel_tempering_chains builds (chain.cc:1330-1340)
  double T = 1;
  for (int i = 0; i < Nt; i++) {
    rung r(1 / T);
    proposal_distribution* c = prop->clone();
    c->set_chain(&r);
    std::vector<double> cum, sc, od;
    if (set->adaptive()) {   // the nested-adaptive recipe: the top thresholds are part of the initial adaptive state
      std::vector<double> w;
      std::vector<int> bits, cnt;
      ((proposal_distribution_set*)c)->adapt_state(w, cum, bits, cnt);
      cum.resize(set->members().size());
    } else if (!c->device_describe_mixture(D, cum, sc, od)) return 5;
    printf("rung %d beta %a :", i, 1 / T);
    for (double v : cum) printf(" %a", v);
    printf("\n");
    delete c;
    T *= tratio;
  }
  return 0;
}
'''


@pytest.fixture(scope="module")
def program():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.cc"), os.path.join(d, "t")
        open(src, "w").write(_PROGRAM)
        r = subprocess.run(["g++", "-std=c++11", "-O1", "-ffp-contract=off", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ptmcmc_amd", "host"),
                            src, "-L", os.path.join(ROOT, "ptmcmc_amd"), "-lptm_engine", "-Wl,-rpath," + os.path.join(ROOT, "ptmcmc_amd"), "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        yield exe


def _run(exe, *flags):
    out = subprocess.run([exe] + list(flags), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    return out.stdout


def _tables(stdout):
    rows = []
    for line in stdout.split("\n"):
        if line.startswith("rung "):
            head, vals = line.split(":")
            rows.append((float.fromhex(head.split()[3]), [float.fromhex(v) for v in vals.split()]))
    return rows


def _recipe_shares(prior_frac, gauss_frac=0.2, nested=False):
    """the sampler's recipe (ptmcmc.cc:60-143): differential evolution 1 - gauss - prior, the prior draws, then the six Gaussians
    2 : 4 : ... : 64 of gauss_draw_frac (one nested member with --prop_adapt_rate); hot shares 0, 1, 0 ..."""
    de = max(0.0, 1 - gauss_frac - prior_frac)
    if nested:
        cold = [de, prior_frac, gauss_frac]
    else:
        total = 2.0 ** 7 - 2
        w, g = 1.0, []
        for _ in range(6):
            w *= 2
            g.append(w / total * gauss_frac)
        cold = [de, prior_frac] + g
    return cold, [0.0, 1.0] + [0.0] * (len(cold) - 2)


def test_the_thermal_recipe_describes_every_rungs_table(program):
    """prior_draw_frac = 0.2, prior_draw_Tpow = 1.5 over 5 rungs: accepted, member 1, every rung's cumulative shares the model's
    reset_bins at that rung's temperature, bit for bit (the last exactly 1)"""
    out = _run(program, "--prior_draw_frac=0.2", "--prior_draw_Tpow=1.5")
    assert "device 1 prior_member 1 fits 1" in out, out[-2000:]
    rows = _tables(out)
    assert len(rows) == 5
    cold, hot = _recipe_shares(0.2)
    for beta, cum in rows:
        _, want = PM.thermal_bins(cold, hot, 1.5, beta)
        want[-1] = 1.0
        assert cum == want, (beta, cum, want)
        assert cum[-1] == 1.0
    assert rows[0][1] != rows[-1][1]
    share = [r[1][1] - r[1][0] for r in rows]
    assert all(b > a for a, b in zip(share, share[1:])) and abs(share[0] - 0.2) < 1e-12   # the prior's share grows towards the hot rungs


def test_the_nested_adaptive_recipe_keeps_its_thermal_top_thresholds(program):
    """--prop_adapt_rate without --prop_adapt_more: the top set does not adapt; its thermal thresholds are the clone's own"""
    out = _run(program, "--prior_draw_frac=0.2", "--prior_draw_Tpow=1.5", "--prop_adapt_rate=0.05")
    assert "device 1 prior_member 1 fits 1" in out, out[-2000:]
    cold, hot = _recipe_shares(0.2, nested=True)
    rows = _tables(out)
    assert len(rows) == 5
    for beta, cum in rows:
        assert cum == PM.thermal_bins(cold, hot, 1.5, beta)[1], (beta, cum)


def test_flat_shares_and_an_adapting_top_set(program):
    # Tpow = 0: one table for every rung
    rows = _tables(_run(program, "--prior_draw_frac=0.2"))
    assert len(rows) == 5 and all(r[1] == rows[0][1] for r in rows)
    # an adapting top set with temperature-dependent shares stays on the host
    out = _run(program, "--prior_draw_frac=0.2", "--prior_draw_Tpow=1.5", "--prop_adapt_rate=0.05", "--prop_adapt_more")
    assert "device 0" in out, out[-2000:]
    # ... and so does everything under PTM_HOST_PRIOR_DRAW=1
    out = subprocess.run([program, "--prior_draw_frac=0.2"], capture_output=True, text=True, timeout=60, env=dict(os.environ, PTM_HOST_PRIOR_DRAW="1"))
    assert out.returncode == 0 and "device 0" in out.stdout, out.stdout[-2000:]
