"""One run of a big-population engine in a process of its own (PTM_ROW_LABELS is read once per process): prints whether the row
labels ever left the identity and a digest of everything the run produced.  usage: python row_labels_worker.py Nt W nsteps"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ptmcmc_amd import engine as E
from ptmcmc_amd.problems import GaussianProblem

if __name__ == "__main__":
    Nt, W, nsteps = (int(v) for v in sys.argv[1:4])
    pr = GaussianProblem(32, Nt, 1e3)
    eng = E.Engine(32, Nt, W, seed=0x5EED0002, swap_rate=0.3)
    pr.configure(eng, E.PROP_LOWER)
    eng.init_from_prior()
    ident = np.repeat(np.arange(Nt, dtype=np.int32), W)
    h = hashlib.sha256()
    used = 0
    for k in range(3):
        eng.step(nsteps); eng.sync()
        used += int((eng.row_labels != ident).any())
        h.update(eng.states().tobytes())
        assert np.array_equal(eng.row_labels, ident)
        for name in ("llike", "lprior", "ntries", "naccept", "last_type", "nhist"):
            h.update(getattr(eng, name).tobytes())
    eng.sweep(1); eng.sync()
    h.update(eng.states().tobytes())
    t, a = eng.swap_counts()
    h.update(np.ascontiguousarray(t).tobytes()); h.update(np.ascontiguousarray(a).tobytes())
    print("ok labels_used=%d digest=%s" % (1 if used else 0, h.hexdigest()))
    eng.close()
