"""The pipelined tile loop of the box pre-pass (ptmcmc_amd/csrc/ptm_box_prefilter.hpp): a block asks for the list entries, rows and
scalars of its later tiles while it draws for the current one, and stores a tile's survivors one tile later.  The shapes of
tests/test_gpu_box_prefilter.py have at most 48 tiles on a grid of about a thousand blocks: no block there sees a second tile.
PTM_PREFILTER_GRID=n caps the grid at n blocks, so here one, two or three blocks walk every tile of every rung, across rung
boundaries with an append pending, through partly filled and idle waves.  Every case runs engine against oracle bit for bit
(tests/box_prefilter_pipeline_worker.py: the cases of box_prefilter_worker.py) with PTM_BOX_PREFILTER=1, in a process of its own;
its counters must be those of the same case on the uncapped grid, and its accepts those of the run without the pre-pass."""
import functools
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def run(case, walkers, setting, grid):
    """one worker run (cached); setting: PTM_BOX_PREFILTER's value, grid: PTM_PREFILTER_GRID's or None for unset"""
    env = dict(os.environ)
    env.pop("PTM_PREFILTER_GRID", None)
    env["PTM_BOX_PREFILTER"] = setting
    if grid is not None:
        env["PTM_PREFILTER_GRID"] = str(grid)
    r = subprocess.run([sys.executable, os.path.join(HERE, "box_prefilter_pipeline_worker.py"), case, str(walkers)], env=env, capture_output=True, text=True, timeout=120)   # (a worker takes about a second: the limit only ends a hung one)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-3000:]
    out = dict(kv.split("=") for kv in r.stdout.split()[1:])
    print(case, walkers, setting, grid, out)
    return {k: int(v) for k, v in out.items()}


# 12 rungs x 1024 walkers at this swap rate list ~600 moving walkers per rung and step: three tiles, the third with one full wave, one
# partly filled and two idle -- one block walks all of them in turn; three blocks: the stride equals a rung's tiles, so a block keeps
# one tile number and the partial tiles meet in one block.  1088 walkers on two blocks (~640 entries, the third tile half full);
# 1344 walkers: ~790 entries with a spread of ~20 around the 768 of three full tiles, so a rung has a fourth tile with a handful of
# entries, or none.  The non-finite starts and both sharded steps (partial sweeps, rung0 != 0) on one block.
CASES = [("lower", 1024, 1), ("lower", 1024, 3), ("lower", 1088, 2), ("lower", 1344, 2),
         ("nonfinite", 1024, 1), ("sharded", 1024, 1), ("sharded_overlap", 1024, 1)]


@pytest.mark.parametrize("case,walkers,grid", CASES)
def test_capped_grid_matches_the_oracle_and_the_uncapped_counters(case, walkers, grid):
    c = run(case, walkers, "1", grid)   # (the worker has compared engine and oracle, or shards and whole ladder, bit for bit)
    free, off = run(case, walkers, "1", None), run(case, walkers, "0", None)
    assert c["eligible"] == 1 and c["rungs_flagged"] == c["rungs"], c
    assert c["seen"] == free["seen"] and c["settled"] == free["settled"], (c, free)   # the counters do not depend on the grid
    assert 0 < c["settled"] < c["seen"], c
    assert off["seen"] == 0 and off["settled"] == 0, off
    assert c["accepts"] > 0 and c["accepts"] == off["accepts"] == free["accepts"], (c, free, off)
