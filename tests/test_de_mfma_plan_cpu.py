"""Differential evolution on the matrix cores without a GPU: when de_mfma_applies (ptmcmc_amd/csrc/ptm_sweep_plan.hpp) hands a sweep to
de_mfma32_kernel -- tests/cxx/de_mfma_plan_main.cc walks the facts and the three values of PTM_DE_MFMA -- and where that kernel was
built: in the engine's own object, under a name the nine per-dimension objects (and with them the census and the sweep plan) never see."""
import glob
import os
import re
import subprocess
import tempfile

from test_sweep_plan_cpu import CSRC, ROOT, _tool, code_object, kernels_of


def test_the_predicate_follows_the_kernels_limits_and_leaves_the_plan_alone():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "de_mfma_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cxx", "de_mfma_plan_main.cc"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    m = re.fullmatch(r"eligible off=(\d+) unset=(\d+) on=(\d+)\n", r.stdout)
    assert m, r.stdout
    off, unset, on = (int(v) for v in m.groups())
    # the walk met populations on both sides of the rule: the properties were not held vacuously
    assert off == 0 and 0 < unset < on, r.stdout


def test_the_four_builds_live_in_the_engines_object_and_nowhere_in_the_per_dimension_ones():
    import __graft_entry__ as G
    G.build_engine()
    objs = sorted(glob.glob(os.path.join(CSRC, "build", "ptm_sweep_dp*.o")))
    assert len(objs) == 9, "the per-dimension objects are missing: %s" % objs
    with tempfile.TemporaryDirectory() as d:
        eng = kernels_of(code_object(os.path.join(CSRC, "build", "ptm_engine.o"), d))
        for kind in (0, 2):
            for ev in ("false", "true"):
                name = "void ptm::de_mfma32_kernel<%d, %s>(ptm::Dev)" % (kind, ev)
                assert name in eng, (name, sorted(k for k in eng if "de_mfma" in k))
        assert len([k for k in eng if "de_mfma" in k]) == 4
        for o in objs:
            syms = subprocess.check_output([_tool("nm"), o], text=True) + "\n".join(kernels_of(code_object(o, d)))
            assert "de_mfma" not in syms, o
