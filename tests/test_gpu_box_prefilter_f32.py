"""The single-precision box pre-pass (ptmcmc_amd/csrc/ptm_box_prefilter.hpp: box_prefilter_f32_kernel), the default wherever the pre-pass
runs; PTM_BOX_PREFILTER_EXACT=1 selects the double-precision kernel it stands in for.  It draws the first 16 normals of a proposal in
float and settles a chain only when the proposal is outside the box by more than a margin (ptm_sweep_plan.hpp: prefilter_margins), so
it may hand a chain to the sweep that the exact kernel would have settled, never the other way round: the chains stay bit for bit
the checker's, and it settles a subset of what the exact kernel settles.

  - the scan behind PTM_BP_DZ: all 2^32 first arguments of Box-Muller for the radius, all 2^32 second ones for sine and cosine, float
    against the sweep's double-precision functions, reduced to maxima on the device;
  - the workers' cases lower / nonfinite / sharded / sharded_overlap (tests/box_prefilter_worker.py through
    box_prefilter_pipeline_worker.py, engine against checker bit for bit) at 12 rungs x 1024 walkers on a grid of 1, 2, 3 blocks and
    uncapped, through both kernels, a process each: the same chains seen, settled_f32 <= settled_exact, and not by much.
"""
import functools
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def test_float_boxmuller_is_within_half_the_margins_dz_of_the_sweeps_for_every_argument():
    """|z_f32 - z| <= |r_f32 - r| |trig_f32| + r |trig_f32 - trig| + the rounding of the float product r_f32 trig_f32, with r <= 6.7637
    and |z_f32| < 8 (half an ulp there: 2^-22).  PTM_BP_DZ is at least twice that; the other half is the room for what no scan covers
    (the double-precision roundings of x + T z in either kernel)."""
    from ptmcmc_amd import engine as E
    s = E.debug_boxmuller_f32_scan()
    print(s)
    assert s["radius_nan"] == 0 and s["trig_nan"] == 0, s
    assert 0.0 < s["max_dr"] < 1e-3 and 0.0 < s["max_dtrig"] < 1e-4, s
    assert s["max_dr"] + 6.76 * s["max_dtrig"] + 2.0 ** -22 <= s["dz"] / 2, s
    assert s["max_r"] <= 6.7637 + s["dz"]


@functools.lru_cache(maxsize=None)
def run(case, exact, grid):
    """one worker run (cached); exact: PTM_BOX_PREFILTER_EXACT set to 1 or absent, grid: PTM_PREFILTER_GRID's value or None for unset"""
    env = dict(os.environ)
    env.pop("PTM_PREFILTER_GRID", None)
    env.pop("PTM_BOX_PREFILTER_EXACT", None)
    env["PTM_BOX_PREFILTER"] = "1"
    if exact:
        env["PTM_BOX_PREFILTER_EXACT"] = "1"
    if grid is not None:
        env["PTM_PREFILTER_GRID"] = str(grid)
    r = subprocess.run([sys.executable, os.path.join(HERE, "box_prefilter_pipeline_worker.py"), case, "1024"], env=env, capture_output=True, text=True, timeout=120)   # (a worker takes about a second: the limit only ends a hung one)
    if r.returncode < 0 or r.returncode in (134, 139):   # a crashed child (abort, fault): start nothing more on the device
        pytest.exit("box_prefilter_pipeline_worker.py %s died (exit %d)\n%s" % (case, r.returncode, r.stderr[-6000:]), returncode=1)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-3000:]
    out = dict(kv.split("=") for kv in r.stdout.split()[1:])
    print(case, "exact" if exact else "f32", grid, out)
    return {k: int(v) for k, v in out.items()}


@pytest.mark.parametrize("grid", [1, 2, 3, None])
@pytest.mark.parametrize("case", ["lower", "nonfinite", "sharded", "sharded_overlap"])
def test_both_kernels_keep_the_checkers_chains_and_the_float_one_settles_a_subset(case, grid):
    f32, exact = run(case, False, grid), run(case, True, grid)   # (each worker has compared engine and checker, or shards and whole ladder, bit for bit)
    for c in (f32, exact):
        assert c["eligible"] == 1 and c["rungs_flagged"] == c["rungs"], c
    assert f32["seen"] == exact["seen"] > 0, (f32, exact)
    assert f32["settled"] <= exact["settled"], (f32, exact)
    # a guard against a margin wrong by an order of magnitude (the error budget predicts a loss near 1 %), not a tuning target
    assert f32["settled"] >= 0.9 * exact["settled"] > 0, (f32, exact)
    assert f32["accepts"] == exact["accepts"] > 0, (f32, exact)
    # the counters do not depend on the grid
    free = run(case, False, None), run(case, True, None)
    assert (f32["seen"], f32["settled"]) == (free[0]["seen"], free[0]["settled"]), (f32, free[0])
    assert (exact["seen"], exact["settled"]) == (free[1]["seen"], free[1]["settled"]), (exact, free[1])
