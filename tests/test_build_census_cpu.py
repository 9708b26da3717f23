"""The census of kernel builds (tests/build_census.py) without a GPU: the table names exactly the sweep and step kernels of the
gfx950 code objects that were built, and the sweep plan (ptmcmc_amd/csrc/ptm_sweep_plan.hpp), asked through
tests/cxx/census_plan_main.cc, chooses for every sweep case the build the case is listed under."""
import glob
import os
import re
import subprocess
import tempfile

import build_census as BC
from test_sweep_plan_cpu import CSRC, ROOT, code_object, kernels_of


def built_names():
    import __graft_entry__ as G
    G.build_engine()
    objs = sorted(glob.glob(os.path.join(CSRC, "build", "ptm_sweep_dp*.o")))
    assert len(objs) == 9, "the per-dimension objects are missing: %s" % objs
    names = []
    with tempfile.TemporaryDirectory() as d:
        for o in objs:
            names += [BC.reported_name(k) for k in kernels_of(code_object(o, d))]
    names = [n for n in names if n]
    assert len(set(names)) == len(names)
    return set(names)


def test_every_built_sweep_and_step_kernel_has_a_case_or_a_reason():
    built = built_names()
    held, not_held = set(BC.CASES), set(BC.NOT_HELD)
    assert not (held & not_held), "listed twice: %s" % sorted(held & not_held)
    assert not (built - held - not_held), "built kernels without a census case: %s" % sorted(built - held - not_held)
    assert not ((held | not_held) - built), "census names that are no built kernel: %s" % sorted((held | not_held) - built)


def test_the_list_of_builds_not_held_stays_short_and_reasoned():
    assert len(BC.NOT_HELD) <= 15
    assert not [n for n in BC.NOT_HELD if "mfma" in n], "a matrix-core build is not held"
    for name, reason in BC.NOT_HELD.items():
        assert isinstance(reason, str) and reason.strip(), name


def test_every_case_names_its_own_configuration():
    """the table's key says what the configuration is for: the padded dimension and the factor's storage of the name are the case's"""
    for name, c in BC.CASES.items():
        DP = BC.padded(c["D"])
        assert c["D"] < DP, (name, "no padded lane")
        if name.startswith("sweep_mfma32"):
            assert DP == 32
        else:
            assert ("mfma%d_" % DP in name) or re.search(r"<%d, " % DP, name), name


def test_the_sweep_plan_chooses_the_build_each_sweep_case_is_listed_under():
    """Every sweep case's SweepFacts follow from its configuration alone (build_census.sweep_facts, the way step_sweep_plan fills them:
    no case is left out); the two step kernels' names are the engine's (ladder_applies, fused_applies need the device's residency
    figures) and are asserted on the GPU only."""
    cases = [(n, c) for n, c in BC.CASES.items() if n.startswith("sweep_")]
    assert len(cases) > 150
    lines = "".join(" ".join(str(v) for v in BC.sweep_facts(c)) + "\n" for _, c in cases)
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "census_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cxx", "census_plan_main.cc"), "-o", exe])
        r = subprocess.run([exe], input=lines, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = r.stdout.splitlines()
    assert len(got) == len(cases)
    wrong = [(n, g, BC.key(c)) for (n, c), g in zip(cases, got) if g != n]
    assert not wrong, wrong
