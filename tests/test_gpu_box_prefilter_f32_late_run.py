"""The box pre-pass late in a run, through both of its kernels (tests/test_gpu_late_run.py holds the other kernels): 12 rungs x 1024
walkers at 32 dimensions, aged after the worker's first leg to PT step 2^32 - 2 with every counter near PTM_COUNT_MAX (tests/aging_util.py),
label-swapping exchange phases, the forced pre-pass on a grid of two blocks.  The single-precision kernel (the default) replays the
sweep's Philox stream at the 64-bit step and adds to ntries up there exactly as the exact one does (PTM_BOX_PREFILTER_EXACT=1): both
runs equal the checker bit for bit, see the same chains, and the float kernel settles a subset."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_runs = {}


def aged(exact):
    if exact not in _runs:
        env = dict(os.environ)
        env.pop("PTM_BOX_PREFILTER_EXACT", None)
        env.update({"PTM_BOX_PREFILTER": "1", "PTM_PREFILTER_GRID": "2"})
        if exact:
            env["PTM_BOX_PREFILTER_EXACT"] = "1"
        r = subprocess.run([sys.executable, os.path.join(HERE, "box_prefilter_worker.py"), "aged"], env=env, capture_output=True, text=True, timeout=300)   # (a worker takes seconds: the limit only ends a hung one)
        if r.returncode < 0 or r.returncode in (134, 139):   # a crashed child (abort, fault): start nothing more on the device
            pytest.exit("box_prefilter_worker.py aged died (exit %d)\n%s" % (r.returncode, r.stderr[-6000:]), returncode=1)
        assert r.returncode == 0 and r.stdout.startswith("ok "), "exit %d\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-6000:])
        _runs[exact] = {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split()[1:])}
        print("exact" if exact else "f32", _runs[exact])
    return _runs[exact]


def test_single_precision_prepass_late_in_a_run():
    c = aged(False)
    assert c["eligible"] == 1 and c["rungs_flagged"] == c["rungs"] == 12 and 0 < c["settled"] < c["seen"] and c["accepts"] > 0, c


def test_exact_prepass_late_in_a_run_settles_a_superset():
    c, f = aged(True), aged(False)
    assert c["eligible"] == 1 and c["rungs_flagged"] == c["rungs"] == 12 and c["accepts"] == f["accepts"] > 0, (c, f)
    assert c["seen"] == f["seen"] and 0.9 * c["settled"] <= f["settled"] <= c["settled"] < c["seen"], (c, f)
