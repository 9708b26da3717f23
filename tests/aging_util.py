"""Puts an engine and its checker twin at a late point of a run: a PT step count near or past 2^32 and chain counters near
PTM_COUNT_MAX = 2^31 - 1, without walking there.

The engine is aged in place through its own checkpoint: d_count is added to every chain's Ntries, Naccept and Nhist, d_count /
add_every_n to the saved row number of every history row, the step count is set, and ptm_restore (+ ptm_set_history, ptm_set_map, the
ladders, the adaptive state) puts it all back.  The checker (oracle/ptm_oracle.c) holds `step` as uint64_t, `nhist` as int64_t and the
other two as int32_t, plain fields that are written here; its row count `nsize` and its linear history rows stay as they are (it
decides "this add saves a row" by nhist % add_every_N and stores it at index nsize: they are decoupled).

d_count is a multiple of add_every_n * capacity: engine row s + d_count / add_every_n then sits in the ring slot row s had, and
checker row s is its partner.  AgedView presents the engine with those known offsets taken off its row counts (nsize, the rows' saved
numbers), so that the comparisons of parity_util / proposal_pairs / census_util are reused as they are; Ntries, Naccept and Nhist are
compared AT their aged values, the checker's being aged too.

Differential evolution draws from rows [0, Nsize): its ring must hold the whole run and may not wrap (ptm_kernels.hpp: de_ready and
the row picks are made from Nhist), so such engines keep their Nhist (shift_nhist=False) and get the step and the Ntries / Naccept
shift only."""
import numpy as np

from ptmcmc_amd import engine as E

COUNT_MAX = E.COUNT_MAX
MARGIN = 16                  # every aged run ends at least this far below COUNT_MAX
ADDS_PER_STEP = 2            # PTM_ADDS_PER_STEP (ptmcmc_amd/csrc/ptm_count_limit.hpp): the most add_state calls of one chain in one PT step
LATE_STEP = 2**32 - 2        # three steps from here cross the 32-bit word boundary of the step number


def largest_shift(top, steps, unit=1, margin=MARGIN):
    """the largest multiple of `unit` (add_every_n * capacity; 1 without a ring) that may be added to counters that stand at `top` at the
    most, so that `steps` more PT steps leave every one of them at or below COUNT_MAX - margin"""
    room = COUNT_MAX - margin - ADDS_PER_STEP * int(steps) - int(top)
    assert room >= unit, (top, steps, unit)
    return room // unit * unit


def checker_counters(lad):
    """writable views of the checker's counters"""
    c, N = lad.s.contents, lad.N
    return (np.ctypeslib.as_array(c.ntries, shape=(N,)), np.ctypeslib.as_array(c.naccept, shape=(N,)), np.ctypeslib.as_array(c.nhist, shape=(N,)))


def age_checker(lad, step, d_count, shift_nhist=True):
    nt, na, nh = checker_counters(lad)
    assert int(nt.max()) + d_count <= COUNT_MAX and int(nh.max()) + d_count <= COUNT_MAX
    nt += np.int32(d_count); na += np.int32(d_count)
    if shift_nhist:
        nh += np.int64(d_count)
    lad.s.contents.step = int(step)


def age_engine(eng, step, d_count, add_every_n=1, shift_nhist=True, adaptive=False):
    """in place, through checkpoint and restore; returns the row offset d_count / add_every_n (0 if Nhist is kept)"""
    assert d_count >= 0 and (not shift_nhist or not eng.hist_rungs or d_count % (add_every_n * eng.hist_cap) == 0), (d_count, add_every_n, eng.hist_cap)
    ada = eng.proposal_adapt_state() if adaptive else None
    ck = eng.checkpoint()
    ck["ntries"] = (ck["ntries"].astype(np.int64) + d_count).astype(np.int32)
    ck["naccept"] = (ck["naccept"].astype(np.int64) + d_count).astype(np.int32)
    d_rows = 0
    if shift_nhist:
        ck["nhist"] = ck["nhist"] + d_count
        d_rows = d_count // add_every_n
        if ck["history"] is not None:
            h = dict(ck["history"])
            h["row"] = np.where(h["row"] >= 0, h["row"].astype(np.int64) + d_rows, h["row"]).astype(np.int32)
            ck["history"] = h
    ck["step"] = int(step)
    eng.restore(ck)
    if ada is not None:
        eng.set_proposal_adapt_state(ada["weights"], ada["thresholds"], ada["repeat_bits"], ada["outcomes"])
    return d_rows


class AgedView:
    """the aged engine with the known row offset taken off its row counts; everything else is the engine's own"""

    def __init__(self, eng, d_rows):
        self._eng, self.d_rows = eng, int(d_rows)

    def __getattr__(self, name):
        return getattr(self._eng, name)

    @property
    def nsize(self):
        return self._eng.nsize - self.d_rows

    def history(self):
        h = dict(self._eng.history())
        h["row"] = np.where(h["row"] >= 0, h["row"].astype(np.int64) - self.d_rows, h["row"])
        return h


def age_pair(eng, lad, steps, step=LATE_STEP, shift_nhist=True, adaptive=False, margin=MARGIN):
    """age the engine and its checker twin alike for `steps` more PT steps (plain sweeps count as steps); returns (view, d_count)"""
    N = int(lad.s.contents.add_every_N)
    unit = N * eng.hist_cap if (shift_nhist and eng.hist_rungs) else 1
    top = max(int(eng.ntries.max()), int(eng.nhist.max()))
    d = largest_shift(top, steps, unit, margin)
    d_rows = age_engine(eng, step, d, N, shift_nhist, adaptive)
    age_checker(lad, step, d, shift_nhist)
    return AgedView(eng, d_rows), d


# ---- differential evolution late in a run -----------------------------------------------------------------------------------------
# Differential evolution draws from every row a chain has saved, so its ring holds the whole run: a run reaches Nhist ~ 2e9 inside a
# ring of a few hundred slots only with a history stride of millions.  add_every_n = 2^24 and DE_ROWS = 128 saved rows put Nhist at
# 127 * 2^24 - 2 = 2130706430: the row picks, the count of saved rows, readiness, parallel and snooker moves all run up there, and the
# third step saves a row.
DE_EVERY, DE_CAP, DE_K = 2**24, 190, 127
DE_NTRIES, DE_NACCEPT = 2000000000, 700000000


def late_de_pair(D, Nt, W, kind, snooker=0.3, ninit=1, K=2, evolve=0.0, **pair_kw):
    """proposal_pairs.de_pair with a history stride of 2^24, both sides handed the same DE_K + 1 invented saved rows (the engine through
    ptm_restore + ptm_set_history, the checker through its hist_* arrays and nsize) and put at PT step 2^32 - 2, Nhist = DE_K * 2^24 - 2"""
    import parity_util as PU
    import proposal_pairs as PP
    pr, eng, lad = PP.de_pair(D, Nt, W, kind, DE_EVERY, snooker, ninit, K, DE_CAP, **pair_kw)
    if evolve:
        eng.set_evolve_temps(evolve); lad.evolve_temps(evolve)
    rows, Nc, cap = DE_K + 1, Nt * W, DE_CAP
    assert ninit * D + rows >= 10 * D, "differential evolution would not be ready"
    rng = np.random.default_rng(D * 131 + Nt)
    h = dict(x=np.zeros((cap, Nc, D)), llike=np.zeros((cap, Nc)), lprior=np.zeros((cap, Nc)), naccept=np.full((cap, Nc), -1, dtype=np.int32),
             ntries=np.full((cap, Nc), -1, dtype=np.int32), last_type=np.full((cap, Nc), -1, dtype=np.int32), row=np.full((cap, Nc), -1, dtype=np.int32),
             invtemp=np.zeros((cap, Nc)))
    h["x"][:rows] = rng.uniform(-1.0, 1.0, size=(rows, Nc, D)) * np.asarray(pr.halfwidths)[None, None, :] * 0.02
    h["llike"][:rows] = -10.0 + rng.normal(size=(rows, Nc))
    h["lprior"][:rows] = eng.lprior[None, :]
    s = np.arange(rows, dtype=np.int64)[:, None]
    h["ntries"][:rows] = (1 + s * (DE_EVERY - 7)).astype(np.int32) + np.zeros((1, Nc), dtype=np.int32)
    h["naccept"][:rows] = (1 + s * (DE_EVERY // 3)).astype(np.int32) + np.zeros((1, Nc), dtype=np.int32)
    h["last_type"][:rows] = rng.integers(0, K + 1, size=(rows, Nc))
    h["row"][:rows] = s.astype(np.int32) + np.zeros((1, Nc), dtype=np.int32)
    h["invtemp"][:] = np.repeat(np.asarray(pr.beta), W)[None, :]
    nhist = DE_K * DE_EVERY - 2
    ck = eng.checkpoint()
    ck["nhist"] = np.full(Nc, nhist, dtype=np.int64)
    ck["ntries"] = np.full(Nc, DE_NTRIES, dtype=np.int32)
    ck["naccept"] = np.full(Nc, DE_NACCEPT, dtype=np.int32)
    ck["step"] = LATE_STEP
    ck["history"] = h
    eng.restore(ck)
    c = lad.s.contents
    assert c.hist_cap == cap
    nt, na, nh = checker_counters(lad)
    nt[:], na[:], nh[:] = DE_NTRIES, DE_NACCEPT, nhist
    np.ctypeslib.as_array(c.nsize, shape=(Nc,))[:] = rows
    to_checker = lambda a: np.stack([PU.to_oracle_order(a[k], Nt, W) for k in range(cap)], axis=1)     # [cap][chain] -> [chain][cap], the checker's chain order
    for name, ptr in (("x", c.hist_x), ("llike", c.hist_ll), ("lprior", c.hist_lp), ("naccept", c.hist_nacc), ("ntries", c.hist_ntry),
                      ("last_type", c.hist_type), ("invtemp", c.hist_beta)):
        a = to_checker(h[name])
        np.ctypeslib.as_array(ptr, shape=a.shape)[:] = a
    c.step = LATE_STEP
    return pr, eng, lad


def run_late_de(eng, lad, steps=12, evolving=False):
    """single PT steps from there, engine against checker after each; both of differential evolution's move types must have been
    accepted (type codes 0 and 10 of member 0), rows were saved, and the run ends 16 below the limit at the least"""
    import parity_util as PU
    PU.assert_same_state(eng, lad, "late differential evolution: set up")
    PU.assert_same_history_and_map(eng, lad, DE_CAP)
    rows0 = eng.nsize.copy()
    assert (rows0 == DE_K + 1).all() and eng.step_count == lad.step == LATE_STEP
    seen = set()
    for k in range(steps):
        eng.step(1); eng.sync(); lad.pt_step(1)
        PU.assert_same_state(eng, lad, "late differential evolution: after %d PT steps" % (k + 1))
        if evolving:
            assert np.array_equal(eng.invtemps(), lad.betaw), k
        seen |= set(int(v) for v in np.unique(eng.last_type))
        if k == 2:
            assert (eng.nsize > rows0).all(), "every chain has saved a row by the third step"
            PU.assert_same_history_and_map(eng, lad, DE_CAP)
    PU.assert_same_history_and_map(eng, lad, DE_CAP)
    assert {0, 10} <= seen and any(v % 10 >= 1 for v in seen), seen
    top = int(max(eng.ntries.max(), eng.nhist.max()))
    assert DE_K * DE_EVERY <= top <= COUNT_MAX - MARGIN, top
    return seen
