"""The box pre-pass's host-side decisions without a GPU (ptmcmc_amd/csrc/ptm_sweep_plan.hpp): tests/cxx/box_prefilter_plan_main.cc holds
SweepPlan::prefilter to the eligibility rules (lower / diagonal / dense factor, bounds, mean, mixture, evolving, tracked, W < 1024)
and the per-rung flag estimate to a Monte-Carlo count, to a factor far inside the box and to one comparable to it."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ptmcmc_amd", "csrc")


def test_prefilter_plan_and_flag_estimate():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "box_prefilter_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cxx", "box_prefilter_plan_main.cc"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
