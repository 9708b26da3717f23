"""The device's nearest-neighbour search (ptm_nn_dist2) against the Python twin of the facade's kl_estimator (tests/kl_model.py), bit
for bit, in a process of its own (PTM_KL_SPLITS, which forces the number of parts the searched set is split into, is read from the
environment).  Prints "ok cases=<n>".
usage: python kl_nn_worker.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ptmcmc_amd import engine as E
import kl_model as K

T = E.load().ptm_nn_dist2_tile()     # the kernel's tile, from the library: the edge sizes below follow it
NP = (1, 2, 63, 64, 65, 257)
NQ = (1, T - 1, T, T + 1, 2 * T + 3)
DIMS = (1, 3, 4, 5, 32, 33, 128)


def check(what, P, Q=None, bounds=(None, None, None)):
    got = E.nn_dist2(P, Q, *bounds)
    want = K.nn_dist2(P, Q, *bounds)
    if not K.same_bits(got, want):
        bad = np.flatnonzero(got != want)
        print("MISMATCH %s: %d of %d queries, first %d: %r != %r" % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]]))
        sys.exit(1)
    return got


def main():
    rng = np.random.default_rng(1234)
    n = 0
    for dim in DIMS:                       # cross-set: every query count with every size of the searched set
        for nP in NP:
            for nQ in NQ:
                check("cross nP=%d nQ=%d dim=%d" % (nP, nQ, dim), rng.standard_normal((nP, dim)), 1.5 * rng.standard_normal((nQ, dim)))
                n += 1
        for nP in NP[1:]:                  # same-set
            check("same nP=%d dim=%d" % (nP, dim), rng.standard_normal((nP, dim)))
            n += 1
    # same-set: where the nearest neighbour lies.  Points far apart on a line, then chosen pairs brought together
    for nP in (2 * T + 3, 257):
        for dim in (1, 5):
            P = np.zeros((nP, dim))
            P[:, 0] = 10.0 * np.arange(nP)
            P[:, -1] += rng.integers(0, 64, nP) / 64.0       # (coarse: the shifts below are exact)
            P[nP - 1] = P[0] + 0.125               # query 0: the last point, in another split than index 0 whenever there are two
            P[T] = P[5] + 0.0625                   # query 5: the first point of the second tile
            P[2 * T] = P[T + 1] - 0.03125          # query T + 1: the first point of the third tile
            got = check("placed nP=%d dim=%d" % (nP, dim), P)
            assert got[0] == dim * 0.125 ** 2 and got[nP - 1] == got[0] and got[5] == dim * 0.0625 ** 2, got[:8]
            n += 1
    P = rng.standard_normal((70, 3))               # duplicates: 0 for both copies, never for a point that has none
    P[40:50] = P[0:10]
    got = check("duplicates", P)
    assert (got[:10] == 0).all() and (got[40:50] == 0).all() and (got[10:40] > 0).all()
    check("duplicates of a searched point", P[:20], P[35:])
    n += 2
    # wrapped dimensions: uniform over the domain (the alternative wins for many pairs), points exactly on either bound
    for dim, wd in ((1, (0,)), (3, (1,)), (5, (0, 4)), (33, (2, 32)), (128, (127,))):
        w, lo, hi = np.zeros(dim, dtype=np.int32), np.zeros(dim), np.zeros(dim)
        P, Q = rng.standard_normal((65, dim)), rng.standard_normal((2 * T + 3, dim))
        for d in wd:
            w[d], lo[d], hi[d] = 1, -1.0, 2.5
            P[:, d], Q[:, d] = rng.uniform(-1, 2.5, 65), rng.uniform(-1, 2.5, 2 * T + 3)
            P[0, d], P[1, d], Q[0, d], Q[1, d] = -1.0, 2.5, 2.5, -1.0
        plain = K.nn_dist2(P, Q)
        got = check("wrapped cross dim=%d" % dim, P, Q, (w, lo, hi))
        assert (got <= plain).all() and (got < plain).any()
        check("wrapped same dim=%d" % dim, P, None, (w, lo, hi))
        n += 2
    print("ok cases=%d" % n)


if __name__ == "__main__":
    main()
