"""ptm_log_evidence on the histories the REAL reference recorded (tests/golden/evidence.json.gz): the recorded ladders of a group are
the walkers of one engine -- every chain's Nhist through ptm_restore, the saved llikes and their row numbers through ptm_set_history
(states and lpriors are arbitrary), an evolving group's temperatures through ptm_set_evolve_temps + ptm_set_invtemps -- and the device
must give the reference's own log_evidence_ratio answers as up / down bit for bit, the totals and counts of tests/evidence_model.py
(which tests/test_evidence_reference_cpu.py pins to the same answers), at every recorded window length."""
import functools
import math

import numpy as np
import pytest

import evidence_model as M
import evidence_reference_util as U
from ptmcmc_amd import engine as E
from ptmcmc_amd.problems import GaussianProblem

pytestmark = pytest.mark.gpu

D = 2


def loaded_engine(g, ladders, cap, first_row=None, de_init_extra=0):
    """an engine whose ring, counters and ladders are the recorded ones (walker w = ladders[w]); nothing is stepped"""
    nt, w_count, a = int(g["Nt"]), len(ladders), int(g["add_every_N"])
    llike, row, nhist, beta = U.pack_ring(g, ladders, cap, first_row)
    nc = nt * w_count
    pr = GaussianProblem(D, nt, float(g["Tmax"]))
    eng = E.Engine(D, nt, w_count, swap_rate=0.3, seed=0xE71DF, add_every_n=a, history_rungs=nt, history_capacity=cap)
    pr.configure(eng, E.PROP_LOWER)
    evolving = g.get("evolve_rate", 0) > 0
    eng.set_ladder([U.num(b) for b in (ladders[0]["invtemp0"] if evolving else ladders[0]["invtemp"])])
    if evolving:
        eng.set_evolve_temps(float(g["evolve_rate"]))
    if de_init_extra:   # further initial draws sit in front of the ring's row 0, outside the ring
        eng.set_proposal_de(0.1, 0.3, 4.0, 0.0, init_rows=np.random.default_rng(5).uniform(-1, 1, size=(de_init_extra, nc, D)))
    eng.init_from_prior()
    ck = eng.checkpoint()
    ck["nhist"] = nhist
    ck["step"] = int(nhist.max())
    if evolving:
        ck["invtemps"] = beta
    filled = row >= 0
    ck["history"] = dict(x=np.zeros((cap, nc, D)), llike=llike, lprior=np.zeros((cap, nc)), naccept=np.where(filled, 1, -1).astype(np.int32),
                         ntries=np.where(filled, 1, -1).astype(np.int32), last_type=np.full((cap, nc), -1, dtype=np.int32), row=row,
                         invtemp=np.repeat(beta.T.reshape(1, nc), cap, axis=0))
    eng.restore(ck)
    assert np.array_equal(eng.nhist, nhist) and np.array_equal(eng.invtemps(), beta)
    h = eng.history()
    assert np.array_equal(h["row"], row) and np.array_equal(h["llike"], llike)
    return eng


def bits_equal(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all((np.isnan(got) & np.isnan(want)) | (got.view(np.uint64) == want.view(np.uint64))))


@functools.lru_cache(maxsize=None)
def model(name, k, ilen):
    """the model's (evidence, up, down, count) of ladder k of a group: computed once, shared by every test"""
    g = U.group(name)
    return U.model_total(g, g["ladders"][k], ilen)


def all_ilens(g):
    return sorted({q["ilen"] for lad in g["ladders"] for q in lad["queries"]})


def check(eng, g, ilen, tile):
    """one call against the recorded ratios (where this ladder recorded this ilen) and the model, every walker; walker w = ladder w % tile"""
    name, nt = g["name"], int(g["Nt"])
    ev, up, down, count = eng.log_evidence(ilen)
    for k in range(tile):
        m_ev, m_up, m_down, m_count = model(name, k, ilen)
        ws = slice(k, eng.W, tile)
        n = len(range(eng.W)[ws])
        assert bits_equal(ev[ws], [m_ev] * n), (name, k, ilen, ev[ws], m_ev)
        assert bits_equal(up[:, ws], np.repeat(np.array(m_up)[:, None], n, 1)) and bits_equal(down[:, ws], np.repeat(np.array(m_down)[:, None], n, 1)), (name, k, ilen)
        assert np.array_equal(count[:, ws], np.repeat(np.array(m_count)[:, None], n, 1)), (name, k, ilen, count[:, ws], m_count)
        for q in g["ladders"][k]["queries"]:
            if q["ilen"] == ilen:   # the reference's own numbers
                rec = [U.num(v) for v in q["ab"]]
                assert bits_equal(up[:, k], rec[0::2]) and bits_equal(down[:, k], [-v for v in rec[1::2]]), (name, k, ilen, up[:, k], down[:, k], rec)
    return ev


def run_group(name, tile_to=None, cap=None, de_init_extra=0, ilens=None):
    g = U.group(name)
    k_count = len(g["ladders"])
    ladders = [g["ladders"][w % k_count] for w in range(tile_to or k_count)]
    newest = max(U.ring_row(g, n - 1) for lad in g["ladders"] for n in lad["Nsize"])
    eng = loaded_engine(g, ladders, cap or newest + 3, de_init_extra=de_init_extra)
    try:
        seen_nan = seen_finite = 0
        for ilen in ilens or all_ilens(g):
            ev = check(eng, g, ilen, k_count)
            seen_nan += int(np.isnan(ev).sum()); seen_finite += int(np.isfinite(ev).sum())
        assert seen_nan and seen_finite
    finally:
        eng.close()
    return newest


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_every_group_gives_the_references_ratios_at_every_recorded_window(name):
    run_group(name)


def test_group_a_tiled_over_several_workgroups():
    run_group("A", tile_to=320)                     # 1280 chains: five workgroups of the ratio kernel, two of the total's


@pytest.mark.parametrize("name", ["A", "D"])
def test_a_wrapped_ring_that_still_holds_the_widest_finite_window(name):
    """capacity = the longest chain's newest row: that chain's row 0 is overwritten (slot = row mod capacity, the checked path runs for
    every chain) and every recorded window is still there -- the widest, ilen = Nhist, starts at row 1"""
    g = U.group(name)
    newest = max(U.ring_row(g, n - 1) for lad in g["ladders"] for n in lad["Nsize"])
    run_group(name, cap=newest)


@pytest.mark.parametrize("name", ["A", "D"])
def test_a_short_ring_every_chain_wrapped_and_the_refusal_of_a_lost_window(name):
    g = U.group(name)
    a = int(g["add_every_N"])
    cap = 50 // a + 3
    top = max(h for lad in g["ladders"] for h in lad["Nhist"])
    assert all(U.ring_row(g, n - 1) >= cap for lad in g["ladders"] for n in lad["Nsize"])
    run_group(name, cap=cap, ilens=[1, 2, 3, 4, 7, 50, top + 1, 10**6])
    lost = min(h for lad in g["ladders"] for h in lad["Nhist"])                   # recorded, finite -- and no longer in this ring
    k_count = len(g["ladders"])
    eng = loaded_engine(g, g["ladders"], cap)
    try:
        nt = int(g["Nt"])
        out = (np.full(k_count, 7.25), np.full((nt - 1, k_count), -3.5), np.full((nt - 1, k_count), 11.0), np.full((nt, k_count), 99, dtype=np.int32))
        with pytest.raises(E.PtmError) as ei:
            eng.log_evidence(lost, out=out)
        assert "ptm error -1" in str(ei.value) and "history_capacity must hold the evidence window" in str(ei.value)
        assert (out[0] == 7.25).all() and (out[1] == -3.5).all() and (out[2] == 11.0).all() and (out[3] == 99).all()
    finally:
        eng.close()


def test_group_b_with_initial_rows_in_front_of_the_ring():
    """initialize(5) in the reference; the engine keeps the four further draws outside the ring (ptm_set_proposal_de, n_init_extra = 4)"""
    assert U.group("B")["Ninit"] == 5
    run_group("B", de_init_extra=4)


def test_the_long_ladders_final_report():
    """the two do_evid ladders (verbose_evid 1 and 0) as the two walkers of one engine, the ring a few rows longer than the last
    window: the reference's own ratios of the last bin bit for bit, and its last printed total"""
    fx = U.load()
    ladders = fx["long"]
    g = ladders[0]
    assert all(lad["Nt"] == g["Nt"] and lad["add_every_N"] == g["add_every_N"] and lad["invtemp"] == g["invtemp"] for lad in ladders)
    ilen, a, nt = g["bin"], g["add_every_N"], g["Nt"]
    cap = ilen // a + 5
    eng = loaded_engine(g, ladders, cap)
    try:
        ev, up, down, count = eng.log_evidence(ilen)
        for w, lad in enumerate(ladders):
            last = lad["reports"][-1]
            assert last["Nhist"] == lad["Nhist"]
            rec = [U.num(v) for v in last["query"]["ab"]]
            assert bits_equal(up[:, w], rec[0::2]) and bits_equal(down[:, w], [-v for v in rec[1::2]]), (w, up[:, w], down[:, w], rec)
            assert "Total log-evidence: " + M.g(ev[w]) == last["lines"][0], (w, ev[w], last["lines"][0])
            m_ev, _, _, m_count = U.model_total(lad, lad, ilen, snap=last)
            assert bits_equal(ev[w], m_ev) and list(count[:, w]) == m_count and all(1998 <= c <= 2000 for c in m_count)
        out = (np.full(2, 7.25), np.full((nt - 1, 2), -3.5), np.full((nt - 1, 2), 11.0), np.full((nt, 2), 99, dtype=np.int32))
        with pytest.raises(E.PtmError) as ei:
            eng.log_evidence(2 * ilen, out=out)                # two bins: the ring holds one
        assert "history_capacity must hold the evidence window" in str(ei.value)
        assert (out[0] == 7.25).all() and (out[1] == -3.5).all() and (out[2] == 11.0).all() and (out[3] == 99).all()
    finally:
        eng.close()
