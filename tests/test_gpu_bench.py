"""bench.py's single-GPU path as the measurement runs it (-m gpu): a plain run times the headline steps only and writes
what the last step computed with --dump-outputs -- the same files for the same arguments, other files for another --steps;
--full adds the companions, the calibration and the CPU baseline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--walkers", "1024"] + list(extra),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_run_dumps_the_same_outputs_for_the_same_arguments(tmp_path):
    a, b, c = (str(tmp_path / k) for k in "abc")
    ra = _bench("--steps", "4", "--warmup", "2", "--dump-outputs", a)
    rb = _bench("--steps", "4", "--warmup", "2", "--dump-outputs", b)
    rc = _bench("--steps", "5", "--warmup", "2", "--dump-outputs", c)
    for r, n in ((ra, 4), (rb, 4), (rc, 5)):
        assert r["steps"] == n and r["ms_per_step"] > 0 and r["value"] > 0
        assert r["unit"] == "MH steps/s" and r["higher_is_better"] is True and r["dtype"] == "f64"
        assert r["calibration"] is None and r["w1"] is None and r["evolving_ladders"] is None and "cpu_baseline" not in r
        assert abs(r["ms_per_step"] - 1e3 * r["config"]["chains"] / r["value"]) < 1e-9 * r["ms_per_step"]
    A, B, C = _load(a), _load(b), _load(c)
    names = {"chain_index", "states", "llike", "lprior", "lpost", "ntries", "naccept", "last_type", "walker_index", "invtemps",
             "swap_tries", "swap_accepts"}
    assert set(A) == set(B) == set(C) == names
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) < 64 << 20
    for k in names:
        assert A[k].dtype == np.float64 and np.array_equal(A[k], B[k]), k
    assert A["states"].shape == (1 << 16, 32) and np.isfinite(A["states"]).all()
    # one more timed step: one more Metropolis move for the chains no exchange touched
    assert np.array_equal(A["chain_index"], C["chain_index"]) and not np.array_equal(A["states"], C["states"])
    assert (C["ntries"] - A["ntries"]).max() == 1 and (C["ntries"] >= A["ntries"]).all()


def test_full_run_keeps_the_companions_and_the_cpu_baseline():
    r = _bench("--steps", "3", "--warmup", "1", "--full")
    assert r["steps"] == 3 and r["ms_per_step"] > 0
    assert r["calibration"]["copy_GBs"] > 0 and "frac_of_measured_copy" in r["roofline"]
    assert r["w1"]["chains"] == 1024 and r["w1"]["value"] > 0 and r["w1_sampler_defaults"]["value"] > 0
    assert r["cpu_baseline"]["value"] > 0 and r["cpu_baseline"]["kind"] in ("reference", "port")
