"""Row labels: in a big-population step (the compacted sweep's conditions, the whole ladder on one engine, at most 65536 walkers)
an accepted exchange swaps the two rungs' 16-bit row labels instead of their 256-byte rows; the compacted sweep finds a chain's
row through its label, and every other reader or writer of the states first gets the rows put back in place (restore_rows_kernel).
Nothing of this may be visible from outside: every case here is bit for bit the CPU oracle's run (parity_util), or -- at a size
the oracle cannot walk -- the run of a process with PTM_ROW_LABELS=0."""
import os
import subprocess
import sys

import numpy as np
import pytest

import parity_util as PU
from ptmcmc_amd import engine as E

pytestmark = pytest.mark.gpu


def _ident(eng):
    return np.repeat(np.arange(eng.Nt, dtype=np.int32), eng.W)


def _labels_in_use(eng):
    """the table as it stands (reading it restores nothing): is some row away from its rung?"""
    lab = eng.row_labels
    # a permutation of the rungs per walker, whatever the exchanges did
    assert np.array_equal(np.sort(lab.reshape(eng.Nt, eng.W), axis=0), _ident(eng).reshape(eng.Nt, eng.W))
    return bool((lab != _ident(eng)).any())


def _check(eng, lad, what):
    """states and scalars against the oracle (reading the states restores the rows), then the table is the identity"""
    PU.assert_same_state(eng, lad, what)
    assert np.array_equal(eng.row_labels, _ident(eng)), what + ": labels after a restore"


@pytest.mark.parametrize("Nt,kind", [(12, E.PROP_LOWER), (64, E.PROP_DENSE)])
def test_labelled_steps_match_the_oracle_with_repeated_restores(Nt, kind):
    """32 dimensions, 1024 walkers, swap rate 0.3, 24 steps; the states are read every 4 steps, so the restore runs six times, each
    from the permutation that four exchange phases left."""
    pr, eng, lad = PU.make_pair(32, Nt, 1024, 1e3, kind=kind, swap_rate=0.3)
    assert eng.sweep_kernel_name.endswith(", 0, false, true>")
    assert not _labels_in_use(eng)
    for k in range(6):
        eng.step(4); eng.sync(); lad.pt_step(4)
        assert _labels_in_use(eng), "the labelled path did not run"
        _check(eng, lad, "after %d steps" % (4 * (k + 1)))
    t, a = eng.swap_counts()
    assert np.array_equal(t, lad.swap_count) and np.array_equal(a, lad.swap_accept_count)
    eng.close()


@pytest.mark.parametrize("kind,ev", [(E.PROP_LOWER, 0.02), (E.PROP_DENSE, 0.05)])
def test_labelled_steps_of_evolving_ladders(kind, ev):
    """the lean build of evolving ladders: the exchange kernel's evolving form permutes labels, the temperatures stay with the rungs"""
    pr, eng, lad = PU.make_pair(32, 16, 1024, 1e3, kind=kind, swap_rate=0.3)
    eng.set_evolve_temps(ev); lad.evolve_temps(ev)
    for k in range(5):
        eng.step(4); eng.sync(); lad.pt_step(4)
        assert _labels_in_use(eng), "the labelled path did not run"
        _check(eng, lad, "after %d steps" % (4 * (k + 1)))
        assert np.array_equal(eng.invtemps(), lad.betaw)
    t, a = eng.swap_counts()
    assert np.array_equal(t, lad.swap_count) and np.array_equal(a, lad.swap_accept_count)
    eng.close()


@pytest.mark.parametrize("kind,odf,with_mean,ev", [(E.PROP_LOWER, 0.0, False, 0.0), (E.PROP_DENSE, 0.4, True, 0.0), (E.PROP_LOWER, 0.3, False, 0.02)])
def test_labelled_steps_of_the_box_bounds_build(kind, odf, with_mean, ev):
    """uniform priors, `limit` / open boundaries, a mean, one-dimensional moves, an evolving ladder: the box-bounds builds' compacted
    sweep takes the rows by label too (narrow limits: a good share of the proposals is invalid)"""
    D, Nt, W = 30, 12, 1024
    rng = np.random.default_rng(36)
    blo = [1 if d % 3 else 0 for d in range(D)]
    bhi = [1 if d % 2 else 0 for d in range(D)]
    bmin = list(rng.uniform(-2.5, -1.5, D)); bmax = list(rng.uniform(1.5, 2.5, D))
    prior = ([1] * D, [0.0] * D, list(rng.uniform(3.0, 6.0, D)))
    x0 = rng.uniform(-1.4, 1.4, size=(Nt * W, D))
    mean = rng.normal(size=D) * 0.1 if with_mean else None
    pr, eng, lad = PU.make_pair(D, Nt, W, 1e3, kind=kind, bounds=(blo, bhi, bmin, bmax), prior=prior, swap_rate=0.3, x0=x0, mean=mean,
                                one_d_frac=(odf if odf > 0 else None))
    if ev:
        eng.set_evolve_temps(ev); lad.evolve_temps(ev)
    assert eng.sweep_kernel_name.endswith(", %d, %s, true>" % (1 if (odf > 0 or with_mean) else 3, "true" if ev else "false"))
    for k in range(5):
        eng.step(4); eng.sync(); lad.pt_step(4)
        assert _labels_in_use(eng), "the labelled path did not run"
        _check(eng, lad, "after %d steps" % (4 * (k + 1)))
        if ev:
            assert np.array_equal(eng.invtemps(), lad.betaw)
    tries, acc = eng.ntries.sum() - eng.Nc, eng.naccept.sum() - eng.Nc
    assert 0 < acc < 0.8 * tries
    eng.close()


def test_labelled_steps_between_other_users_of_the_rows():
    """Plain sweeps (no exchange phase: every chain in place), ptm_set_states on an engine whose rows are away from their rungs, a
    checkpoint restored into a second engine, and one into an engine that records a history and a MAP (an engine's history is fixed
    when it is created: this is how a run switches it on) -- each takes the rows through the accessor that restores them first."""
    D, Nt, W, sr, kind = 32, 12, 1024, 0.3, E.PROP_LOWER
    pr, eng, lad = PU.make_pair(D, Nt, W, 1e3, kind=kind, swap_rate=sr)
    x0 = eng.states()
    eng.step(3); eng.sync()
    assert _labels_in_use(eng)
    eng.set_states(x0)                                # the run starts over: counters and step count too (the oracle has not moved yet)
    assert np.array_equal(eng.row_labels, _ident(eng))
    _check(eng, lad, "after set_states")
    t0, a0 = eng.swap_counts()                        # (the swap counters are not the states': they keep counting)
    eng.step(5); eng.sync(); lad.pt_step(5)
    assert _labels_in_use(eng)
    eng.sweep(2); eng.sync(); lad.sweep(2)            # plain sweeps straight after labelled steps, nothing read in between
    assert np.array_equal(eng.row_labels, _ident(eng))
    _check(eng, lad, "after plain sweeps")
    eng.step(4); eng.sync(); lad.pt_step(4)
    assert _labels_in_use(eng)
    ck = eng.checkpoint()                             # reads the states: restores
    assert np.array_equal(eng.row_labels, _ident(eng))
    e2 = E.Engine(D, Nt, W, swap_rate=sr)
    pr.configure(e2, kind)
    e2.restore(ck)
    e3 = E.Engine(D, Nt, W, swap_rate=sr, history_rungs=Nt, history_capacity=8, map_rungs=Nt)
    pr.configure(e3, kind)
    e3.restore(ck)
    for e in (eng, e2, e3):
        e.step(5); e.sync()
    lad.pt_step(5)
    assert _labels_in_use(eng) and _labels_in_use(e2)
    assert not _labels_in_use(e3)                     # history / MAP: rows move
    _check(eng, lad, "after 14 steps")
    _check(e2, lad, "resumed engine")
    xe = e3.states()
    assert np.array_equal(xe, eng.states()) and np.array_equal(e3.llike, eng.llike) and np.array_equal(e3.naccept, eng.naccept)
    m = e3.map()
    assert np.isfinite(m["lpost"]).all()
    t, a = eng.swap_counts()
    assert np.array_equal(t - t0, lad.swap_count) and np.array_equal(a - a0, lad.swap_accept_count)
    for e in (eng, e2, e3):
        e.close()


def test_label_overflow_path_many_moved_rows():
    """More than 256 rows of one ladder change rungs in one step (900 rungs, swap rate 0.45): the exchange kernel's cycle walk
    carries the label along with the scalars."""
    pr, eng, lad = PU.make_pair(32, 900, 1024, 1e3, kind=E.PROP_LOWER, swap_rate=0.45)
    moved_max = 0
    for k in range(3):
        eng.step(1); eng.sync(); lad.pt_step(1)
        assert _labels_in_use(eng)
        moved_max = max(moved_max, int(2 * eng.last_swaps()[1].sum(axis=1).max()))
        _check(eng, lad, "after step %d" % (k + 1))
    assert moved_max > 256, moved_max
    eng.close()


def test_switched_off_labels_give_identical_arrays():
    """128 rungs x 2048 walkers, each build in a process of its own: PTM_ROW_LABELS=0 moves rows as ever, the default exchanges
    labels; states, scalars, counters and swap bookkeeping (a digest over three read-backs and a plain sweep) are the same bytes."""
    here = os.path.dirname(os.path.abspath(__file__))
    outs = []
    for env in ({}, {"PTM_ROW_LABELS": "0"}):
        r = subprocess.run([sys.executable, os.path.join(here, "row_labels_worker.py"), "128", "2048", "5"],
                           env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-3000:]
        outs.append(dict(kv.split("=") for kv in r.stdout.split()[1:]))
    assert outs[0]["labels_used"] == "1" and outs[1]["labels_used"] == "0", outs
    assert outs[0]["digest"] == outs[1]["digest"], outs
