"""The single-precision box pre-pass's margin without a GPU (ptmcmc_amd/csrc/ptm_sweep_plan.hpp: prefilter_margin, prefilter_margins):
tests/cxx/box_prefilter_margin_main.cc draws lower-triangular and diagonal factors from 1e-33 to 1e33 with zero rows, normals up to
6.76 that are off by up to PTM_BP_DZ, multiplies them in float in three orders and four ways of summing, and holds the distance to the
double-precision product under m_d; the margin is 0 for a zero row, infinite for a row float cannot hold, and monotone in |T|."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ptmcmc_amd", "csrc")


def test_float_product_stays_within_the_margin():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "box_prefilter_margin")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cxx", "box_prefilter_margin_main.cc"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-4000:]
