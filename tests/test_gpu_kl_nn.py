"""The exact nearest-neighbour search of the k-NN KL estimator on the device (ptm_nn_dist2, ptmcmc_amd/csrc/ptm_kl_kernels.hpp) against
the Python twin of the facade's kl_estimator (tests/kl_model.py), bit for bit -- every size around a workgroup and a tile, every
padded dimension, same-set searches with the neighbour in chosen places, wrapped dimensions, with the searched set split 1, 2 and 7
ways and as the engine chooses (tests/kl_nn_worker.py, a process per PTM_KL_SPLITS) --, the refused arguments, and the KL value of
the real reference's recorded pairs (tests/golden/kl_divergence.json.gz)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kl_model as K
from ptmcmc_amd import engine as E

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("splits", [None, "1", "2", "7"])
def test_nn_dist2_carries_the_estimators_bits(splits):
    env = dict(os.environ)
    env.pop("PTM_KL_SPLITS", None)
    if splits is not None:
        env["PTM_KL_SPLITS"] = splits
    r = subprocess.run([sys.executable, os.path.join(HERE, "kl_nn_worker.py")], env=env, capture_output=True, text=True, timeout=300)   # (a worker takes a few seconds: the limit only ends a hung one)
    if r.returncode < 0 or r.returncode in (134, 139):   # a crashed child (abort, fault): start nothing more on the device
        pytest.exit("kl_nn_worker.py died (exit %d)\n%s" % (r.returncode, r.stderr[-6000:]), returncode=1)
    print(splits, r.stdout[-500:])
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-3000:]


def refused(code, *args, **kw):
    out = np.full(len(args[0]) if len(args) else 1, -7.0)
    with pytest.raises(E.PtmError, match="ptm error %d:" % code):
        E.nn_dist2(*args, out=out, **kw)
    assert (out == -7.0).all()              # outputs untouched


def test_refused_arguments_leave_the_output_alone():
    rng = np.random.default_rng(3)
    P, Q = rng.standard_normal((9, 3)), rng.standard_normal((5, 3))
    refused(-2, rng.standard_normal((9, 129)), rng.standard_normal((5, 129)))                   # PTM_ERR_UNSUPPORTED: dim > 128
    refused(-1, P[:1])                                                                          # same_set with nP < 2
    refused(-1, np.zeros((0, 3)), Q)                                                            # nP < 1
    refused(-1, P, np.zeros((0, 3)))                                                            # nQ < 1
    refused(-1, np.zeros((4, 0)), np.zeros((4, 0)))                                             # dim < 1
    for lo, hi in ((1.0, 1.0), (2.0, 1.0)):                                                     # a wrapped dimension with xmax <= xmin
        refused(-1, P, Q, wrapped=[0, 1, 0], xmin=[0, lo, 0], xmax=[0, hi, 0])
    for bad in (np.nan, np.inf, -np.inf):                                                       # a non-finite coordinate in either set
        X = P.copy()
        X[8, 2] = bad
        refused(-1, X, Q)
        refused(-1, X)
        Y = Q.copy()
        Y[0, 0] = bad
        refused(-1, P, Y)
    L, nul, out = E.load(), None, np.full(9, -7.0)
    for args in ((nul, 9, E._d(Q), 5, 3, nul, nul, nul, 0, E._d(out)), (E._d(P), 9, nul, 5, 3, nul, nul, nul, 0, E._d(out)),
                 (E._d(P), 9, E._d(Q), 5, 3, nul, nul, nul, 0, nul), (E._d(P), 9, E._d(Q), 5, 3, nul, nul, nul, 1, E._d(out))):
        assert L.ptm_nn_dist2(-1, *args) == -1                                                  # null arguments; same_set with nQ != nP
    assert (out == -7.0).all()
    assert K.same_bits(E.nn_dist2(P, Q, out=out), K.nn_dist2(P, Q)) and (out >= 0).all()        # ... and the call that is right fills it


@pytest.mark.parametrize("name", [c["name"] for c in K.load()["cases"]])
def test_kl_divergence_equals_the_references_recorded_value(name):
    c = next(c for c in K.load()["cases"] if c["name"] == name)
    assert K.same_bits(E.nn_dist2(c["P"], None, *c["bounds"]), c["r1sqs"])
    assert K.same_bits(E.nn_dist2(c["P"], c["Q"], *c["bounds"]), c["s1sqs"])
    got = E.kl_divergence(c["P"], c["Q"], *c["bounds"])
    assert K.same_bits(got, c["kl"]), (got, c["kl"])
