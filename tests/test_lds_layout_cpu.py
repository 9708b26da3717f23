"""The kernels' LDS layouts (ptmcmc_amd/csrc/ptm_lds_layout.hpp) without a GPU: tests/cxx/lds_layout_main.cc carves every layout over
the shapes it lists, checks that each is well formed (regions inside the allocation, aligned, disjoint but for declared reuse; both
sides of the exchange kernel's alias rule among the shapes) and prints the byte count of every shape; each must be the one the
hand-written byte-count functions gave before the layouts replaced them (tests/golden/lds_bytes.json).  Where the compiler's sanitizer
runtime is installed the program also runs under -fsanitize=address,undefined."""
import json
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ptmcmc_amd", "csrc")


def test_every_lds_layout_is_well_formed_and_as_large_as_it_was():
    with open(os.path.join(ROOT, "tests", "golden", "lds_bytes.json")) as f:
        want = json.load(f)["rows"]
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "lds_layout")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cxx", "lds_layout_main.cc"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        # the same program under the address and undefined-behaviour sanitizers, where this machine's compiler has their runtime: it
        # writes every region of every layout over a heap buffer of exactly `bytes`
        san = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                              os.path.join(ROOT, "tests", "cxx", "lds_layout_main.cc"), "-o", exe + "_san"], capture_output=True, text=True)
        if san.returncode == 0:
            rs = subprocess.run([exe + "_san"], capture_output=True, text=True, timeout=300)
            assert rs.returncode == 0 and rs.stdout == r.stdout, rs.stderr[-2000:]
    assert r.returncode == 0, r.stderr     # the properties, checked inside the program
    got = json.loads(r.stdout)["rows"]
    assert len(want) > 400 and sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, "LDS sizes that changed (now, before): %s" % wrong
