"""The proposal test on the device (ptmcmc_amd.engine.proposal_invariance) for three proposals, in a process of its own: torch is
imported before the engine library (one HIP runtime per process, see Engine.set_proposal_device).  Prints one JSON object:
{"native" | "device" | "contraction": the result dict, arrays as lists}.
usage: python proposal_test_worker.py"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ptmcmc_amd import engine as E

DIM, NSAMP, NCYC, NTRY = 3, 2048, 10, 4
CENTRE, SIGMA = np.array([3.0, 0.0, -2.0]), np.array([0.4, 0.5, 2.0])
# dimension 0 wraps around [0, 2 pi) (the target sits 7 sigma inside); dimension 1 ends at a lower limit 1.2 sigma below the centre (the
# origin stays inside: Gaussian steps are built on the space's enforced origin, as in the reference)
BOUNDS = ([E.BOUND_WRAP, E.BOUND_LIMIT, E.BOUND_OPEN], [E.BOUND_WRAP, E.BOUND_OPEN, E.BOUND_OPEN], [0.0, -0.6, 0.0], [2 * np.pi, 0.0, 0.0])
SEED = 20191


def native_gaussian(eng):
    eng.set_proposals(E.PROP_DIAG, 0.7 * SIGMA)


def symmetric_device(eng):
    scale = torch.tensor(0.7 * SIGMA, dtype=torch.float64, device="cuda")

    def propose(x_cur, rung, walker, count, step, x_prop, log_hastings, kind, valid):
        x_prop.copy_(x_cur + scale * torch.randn_like(x_cur))       # symmetric: log-Hastings 0, as preset
    eng.set_proposal_device(propose)


def contraction_device(eng):
    centre = torch.tensor(CENTRE, dtype=torch.float64, device="cuda")

    def propose(x_cur, rung, walker, count, step, x_prop, log_hastings, kind, valid):
        x_prop.copy_(centre + 0.9 * (x_cur - centre))               # always uphill and its ratio claimed to be 0: always accepted
    eng.set_proposal_device(propose)


INSTALL = {"native": native_gaussian, "device": symmetric_device, "contraction": contraction_device}


def main():
    out = {}
    for which in ("native", "device", "contraction"):
        torch.manual_seed(7)
        r = E.proposal_invariance(DIM, CENTRE, SIGMA, INSTALL[which], nsamp=NSAMP, ncyc=NCYC, ntry=NTRY, bounds=BOUNDS, seed=SEED)
        out[which] = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in r.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
