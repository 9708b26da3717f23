"""One run of box_prefilter_worker's cases at a chosen number of walkers per rung, in a process of its own (PTM_BOX_PREFILTER and
PTM_PREFILTER_GRID are read once per process): with the pre-pass's grid capped at a few blocks every block walks many tiles, which
is what the pipelined tile loop of ptmcmc_amd/csrc/ptm_box_prefilter.hpp does on a big population.  Prints the pre-pass's counters
and the Metropolis accepts of every engine of the run.
usage: python box_prefilter_pipeline_worker.py lower|nonfinite|sharded|sharded_overlap [walkers]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ptmcmc_amd import engine as E
import box_prefilter_worker as BW
from box_prefilter_worker import run_pair, run_nonfinite, run_sharded

accepts = 0
_close = E.Engine.close


def counting_close(self):
    """the accepts of every engine of the run, read as it is closed (the sharded cases close theirs themselves)"""
    global accepts
    if getattr(self, "h", None):
        accepts += int(self.naccept.sum() - self.Nc)
    _close(self)


if __name__ == "__main__":
    case = sys.argv[1]
    if len(sys.argv) > 2:
        BW.W = int(sys.argv[2])
    E.Engine.close = counting_close
    if case == "lower":
        res = run_pair(E.PROP_LOWER)
    elif case == "nonfinite":
        res = run_nonfinite()
    elif case in ("sharded", "sharded_overlap"):
        res = run_sharded(case == "sharded_overlap")
    else:
        raise SystemExit("unknown case " + case)
    res = " ".join(kv for kv in res.split() if not kv.startswith("accepts="))
    print("ok " + res + " accepts=%d" % accepts)
