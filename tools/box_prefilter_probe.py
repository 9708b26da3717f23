"""The box pre-pass on the benchmark's workload: after bench.py's settling steps, what share of the chains it sees does it settle,
how many rungs are flagged, and what do the step and the sweep kernel take?  One JSON line.  Run it once per setting of
PTM_BOX_PREFILTER (read once per process): =1 for the share on every rung, unset for what the estimate flags, =0 for the step without.
usage: python tools/box_prefilter_probe.py [steps]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from ptmcmc_amd import engine as E
from ptmcmc_amd.problems import GaussianProblem

if __name__ == "__main__":
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    W = bench.DEFAULT_WALKERS
    pr = GaussianProblem(bench.D, bench.NT, bench.TMAX)
    eng = E.Engine(bench.D, bench.NT, W, seed=bench.SEED, swap_rate=bench.SWAP_RATE, add_every_n=100, time_kernels=True)
    pr.configure(eng, E.PROP_LOWER)
    eng.init_from_prior()
    n_settle = bench.settle_steps(bench.NT * W)
    bench.settle(eng, n_settle)
    bench.settle(eng, n_settle)
    eng.step(10)
    c0, t0 = eng.prefilter_counts(), eng.counter_sums()[0]
    eng.kernel_times(drop=True)
    eng.sync()
    eng.timer_start()
    eng.step(steps)
    ms = eng.timer_stop()
    eng.sync()
    kt = eng.kernel_times()
    c1, t1 = eng.prefilter_counts(), eng.counter_sums()[0]
    seen, settled, moved = (c1["seen"] - c0["seen"]) / steps, (c1["settled"] - c0["settled"]) / steps, (t1 - t0) / steps
    print(json.dumps({"setting": os.environ.get("PTM_BOX_PREFILTER"), "steps": steps, "rungs_flagged": c1["rungs_flagged"], "eligible": c1["eligible"],
                      "moving_chains_per_step": moved, "seen_per_step": seen, "settled_per_step": settled,
                      "settled_share_of_seen": settled / seen if seen else None, "settled_share_of_moving": settled / moved,
                      "swept_chains_per_step": moved - settled, "device_ms_per_step": ms / steps, "sweep_kernel_ms": float(kt.mean()),
                      "sweep_ns_per_chain": float(kt.mean()) * 1e6 / (moved - settled), "kernel": eng.sweep_kernel_name}))
    eng.close()
