"""Times ptm_log_evidence (Engine.log_evidence: two kernels on the device's own history ring, every walker's ladder at once) against
what the host path has to do first -- read the ring's llikes and row numbers of every rung back (ptm_get_history_chains, the
read-back of the facade's PTM_HOST_EVIDENCE=1 path) -- and a one-core pass over them (numpy's column sums: a lower bound of the
sequential evidence_estimator).  Shapes: 20 rungs x 1 walker, 20 x 64, 128 x 512.  Writes profiles/evidence_device.json.

    python tools/evidence_probe.py [steps] [repeats]      (default 1000 steps, window = steps; 5 repeats, the best one counts)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ptmcmc_amd import engine as E  # noqa: E402
from ptmcmc_amd.problems import GaussianProblem  # noqa: E402


def best(f, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        out.append(time.perf_counter() - t0)
    return min(out) * 1e3


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    rows = []
    for Nt, W in ((20, 1), (20, 64), (128, 512)):
        D = 4
        pr = GaussianProblem(D, Nt, 1e4)
        eng = E.Engine(D, Nt, W, swap_rate=0.01, history_rungs=Nt, history_capacity=2 * steps + 4)
        pr.configure(eng, E.PROP_LOWER)
        eng.init_from_prior()
        eng.step(steps)
        eng.sync()
        ev = eng.log_evidence(steps)[0]
        cap, HC = eng.hist_cap, Nt * W
        ll, meta = np.empty((cap, HC)), np.empty((cap, HC, 4), dtype=np.int32)
        eng.L.ptm_get_history_chains.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]

        def read_back():
            E._chk(eng.L.ptm_get_history_chains(eng.h, 0, HC, None, ll.ctypes.data, None, meta.ctypes.data, None))
        t_dev = best(lambda: eng.log_evidence(steps), repeats)
        t_read = best(read_back, repeats)
        t_sum = best(lambda: (ll[1:steps].sum(axis=0), (meta[1:steps, :, 3] >= 0).all()), repeats)
        rows.append(dict(rungs=Nt, walkers=W, chains=HC, window_steps=steps, ring_rows=cap, device_ms=t_dev, host_read_back_ms=t_read,
                         host_one_core_sum_ms=t_sum, finite=bool(np.isfinite(ev).all())))
        print(rows[-1], flush=True)
        eng.close()
    out = os.path.join(ROOT, "profiles", "evidence_device.json")
    json.dump(dict(what="ptm_log_evidence against the read-back and one-core pass of the host path; host clock around the call, best of %d" % repeats,
                   cases=rows), open(out, "w"), indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
