"""What tests/test_gpu_history_readers.py relies on, checked without a GPU on the same rings from the CPU checker (its ring is the
engine's bit for bit: test_history_rows_match_the_oracle): the queries of every permuted ring can tell a wrong row position from the
right one, the rings fit their capacities, walkers of a rung differ in their add_state counts, and the ilen sweep meets windows that
are empty for some chains of a call and full for others."""
import functools

import numpy as np
import pytest

import history_readers_util as U


@functools.lru_cache(maxsize=None)
def checker(name):
    """ring `name` from the CPU checker, every rung recorded in a ring that keeps the whole run"""
    ring = U.RINGS[name]
    hist, nhist, beta, nsize = U.oracle_of(ring, rungs=ring.Nt)
    return ring, hist, nhist, beta, nsize


def test_row_pos_is_a_permutation_of_every_block_of_eight_that_moves_all_but_its_ends():
    for f in range(128):
        assert U.row_pos(f) // 8 == f // 8
        assert (U.row_pos(f) == f) == (f % 8 in (0, 7))
    assert sorted(U.row_pos(f) for f in range(128)) == list(range(128))


@pytest.mark.parametrize("name", list(U.RINGS))
def test_the_ring_fits_and_walkers_of_a_rung_differ(name):
    ring, hist, nhist, beta, nsize = checker(name)
    assert nsize[:ring.hist_rungs * ring.W].max() <= ring.cap, (ring.name, int(nsize.max()))
    nh = nhist.reshape(ring.Nt, ring.W)
    assert (nh >= ring.steps).all()
    assert len(set(nh[1].tolist())) > 1, (ring.name, nh[1])
    for width, every, burn in ring.shapes:               # at least three windows for the shortest series
        assert ring.steps // ((width // every) * every) - burn >= 3
    assert ring.shapes[0][1] % ring.add == 0 and (ring.add == 1 or ring.shapes[1][1] % ring.add != 0)
    assert (ring.shapes[2][0] // ring.shapes[2][1]) * ring.shapes[2][1] < ring.shapes[2][0]
    assert 1 in U.ess_rungs(ring) and 0 in U.ess_rungs(ring) and ring.hist_rungs - 1 in U.ess_rungs(ring)


def informative(k, D):
    """does the identity in place of row_pos read another SET of features at nfeat = k?  (the answer is a minimum over the features
    looked at: a permutation of them inside the first k positions changes nothing)"""
    dp = 32 if D <= 32 else 64 if D <= 64 else 128
    inv = {U.row_pos(f): f for f in range(dp)}
    return {inv[p] for p in range(k) if inv[p] < D} != set(range(k))


def test_which_nfeat_can_see_a_wrong_position():
    assert [k for k in range(1, 13) if informative(k, 21)] == [2, 3, 4, 5, 6, 10, 11, 12]
    # nfeat = D: whole blocks of eight hold the same features either way; only a last, partial block differs, by at most two features
    assert not informative(32, 32) and not informative(17, 17) and not informative(40, 40) and all(informative(D, D) for D in (20, 21, 100))


@pytest.mark.parametrize("name", [r.name for r in U.RINGS.values() if r.permuted])
def test_a_wrong_row_position_changes_an_answer_the_gpu_test_sees(name):
    """The mistake a broken ess_pos would make is the identity in place of row_pos: feature f read from position f of the stored row.
    The answer is the minimum over the features looked at, so the mistake shows where it changes the SET of features read and one of
    the features that left or joined decides a walker's minimum.  At nfeat = D the sets differ by the two features at most that a last,
    partial block of eight loses to its padding lanes (1 of 21 on ring A: 124 of 1920 walker-queries measured, none at all on ring C, whose
    40 dimensions fill their blocks -- no seed, width or step count changes that count of features, so half of the walkers is out
    of reach there); the queries that cut inside a block (nfeat 2..6, 10..12) swap up to half
    of the features, and they are where the bound of one half is held: on every rung and window shape, at least half of the walkers
    get another answer at one of the queried nfeat."""
    ring, hist, nhist, beta, nsize = checker(name)
    moved, at_D = set(), 0
    for rung in U.ess_rungs(ring):
        true = U.EssModel(hist, nhist, ring.W, rung, ring.add, ring.D)
        broken = U.EssModel(hist, nhist, ring.W, rung, ring.add, ring.D, stored_order=True)
        for shape in ring.shapes:
            last, seen = None, np.zeros(ring.W, dtype=bool)
            for k in U.nfeats(ring):
                ans, bad = true.windowed(k, *shape), broken.windowed(k, *shape)
                assert (ans[1] > 0).all()
                if last is not None and k <= 12 and not (U.same_bits(ans[0], last[0]) and np.array_equal(ans[1], last[1])):
                    moved.add(k)                          # the answer at nfeat = k is not the answer at nfeat = k - 1
                last = ans
                differ = (ans[0].view(np.uint64) != bad[0].view(np.uint64)) | (ans[1] != bad[1])
                assert informative(k, ring.D) or not differ.any()
                seen |= differ
                if k == ring.D:
                    at_D += int(differ.sum())
                print(ring.name, "rung", rung, shape, "nfeat", k, "walkers with another answer:", int(differ.sum()), "of", ring.W)
            assert 2 * int(seen.sum()) >= ring.W, (ring.name, rung, shape, int(seen.sum()))
    # for at least two k >= 2 whose newest feature sits at another position than its index, that feature decides an answer
    assert len([k for k in moved if U.row_pos(k - 1) != k - 1]) >= 2, (ring.name, sorted(moved))
    print(ring.name, "nfeat = D: another answer in", at_D, "of", ring.W * len(U.ess_rungs(ring)) * len(ring.shapes), "walker-queries")


def test_the_ilen_sweep_meets_windows_empty_for_some_chains_and_full_for_others():
    s = U.SWEEP
    hist, nhist, beta, nsize = U.oracle_ring(s["D"], s["Nt"], s["W"], "lower", s["add"], s["seed"], s["swap_rate"], s["steps"], s["Nt"])
    assert nsize.max() <= s["cap"]
    lo, hi = int(nhist.min()), int(nhist.max())
    assert lo == s["steps"] and hi > lo + 1
    mixed = 0
    for ilen in U.sweep_ilens(nhist):
        ev, up, down, count = U.evidence_model(hist, nhist, beta, s["Nt"], s["W"], ilen, s["add"])
        empty = nhist.reshape(s["Nt"], s["W"]) < ilen
        assert np.array_equal(count == 0, empty)
        # a ratio is NaN exactly where the chain it reads has an empty window
        assert np.array_equal(np.isnan(up), empty[1:]) and np.array_equal(np.isnan(down), empty[:-1])
        mixed += bool(empty.any() and not empty.all())
    assert mixed >= 1


def test_the_combined_edges_case_has_all_its_edges():
    c = U.EDGES
    hist, nhist, beta, nsize = U.oracle_ring(c["D"], c["Nt"], c["W"], "lower", c["add"], c["seed"], c["swap_rate"], c["steps"], c["Nt"], evolve=c["evolve"])
    assert nsize.min() > c["cap"]                                                  # wrapped
    assert c["ilen"] % c["add"] and len(set(nhist.tolist())) > 3
    assert not np.array_equal(beta[0], beta[1])                                    # the ladders have evolved apart
    ev, up, down, count = U.evidence_model(U.wrapped(hist, nsize, c["cap"]), nhist, beta, c["Nt"], c["W"], c["ilen"], c["add"])
    assert np.isfinite(ev).all() and (count > 0).all() and (count % 8 != 0).all() and len(set(count.ravel().tolist())) > 1
    assert count.max() + 1 <= c["cap"]                                             # the window and the newest row are still there


def test_ring_A_evidence_window_fits_its_short_wrapped_ring():
    ring = U.RINGS["A"]
    ring, hist, nhist, beta, nsize = checker("A")
    assert nsize.min() > U.A_EVIDENCE_CAP
    ev, up, down, count = U.evidence_model(U.wrapped(hist, nsize, U.A_EVIDENCE_CAP), nhist, beta, ring.Nt, ring.W, ring.ilen, ring.add)
    assert np.isfinite(ev).all() and (count == ring.ilen - 1).all()
