"""The box pre-pass's tile-to-rung lookup without a GPU (ptmcmc_amd/csrc/ptm_sweep_plan.hpp: prefilter_slice, the one function the
kernel asks for the tile it works on and for the tiles it loads ahead): tests/cxx/box_prefilter_tiles_main.cc holds it to a linear
walk over lists with empty rungs at the start, in the middle and at the end, and to 'past the end' from ntiles on."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ptmcmc_amd", "csrc")


def test_prefilter_slice_against_a_linear_walk():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "box_prefilter_tiles")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cxx", "box_prefilter_tiles_main.cc"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
