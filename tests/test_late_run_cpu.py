"""Late in a run, without a GPU: what tests/test_gpu_late_run.py rests on.

  - counters shifted by aging_util leave the checker's chains alone (so an aged GPU case cannot fail by the ageing itself);
  - a step number that lost its high word walks other chains at once (so an aged GPU case cannot pass with a 32-bit step anywhere);
  - the counter layout of the random streams at the edges of the step's two words, against a restatement of Philox4x32-10 written
    here and pinned by the Random123 known answers;
  - the horizon's arithmetic (ptmcmc_amd/csrc/ptm_count_limit.hpp) in a stand-alone program under the sanitizers."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import aging_util as AU
import oracle_lib as O
import parity_util as PU
from ptmcmc_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ptmcmc_amd", "csrc")
SEED = 0x5EED0001
D, NT, W = 5, 4, 3


def checker(N=1, cap=0, evolve=0.0, mix=0, step=0):
    """a small ladder population of the checker: history of every N-th add (cap > 0), evolving ladders, a scale mixture"""
    pr = PU.problem_for(D, NT, 1e2)
    lad = O.Ladder(PU.oracle_problem(pr), pr.beta, W=W, swap_rate=0.3, add_every_N=N)
    fac = pr.proposal_factors()
    lad.set_proposals([(O.PROP_DENSE, fac[r], 0.0) for r in range(NT)])
    if mix:
        shares = 2.0 ** np.arange(1, mix + 1)
        cum = np.tile(np.cumsum(shares) / shares.sum(), (NT, 1)); cum[:, -1] = 1.0
        lad.set_mixture(cum, np.tile(3.0 ** -np.arange(mix)[::-1] * 1.2, (NT, 1)), np.tile(np.where(np.arange(mix) % 2 == 0, 0.4, 0.0), (NT, 1)))
    lad.use_philox(SEED)
    if cap:
        lad.enable_history(cap)
    rng = np.random.default_rng(11)
    lad.set_states(rng.uniform(-0.8, 0.8, size=(NT * W, D)) * np.sqrt(np.diag(pr.cov)))
    if evolve:
        lad.evolve_temps(evolve)
    lad.s.contents.step = step
    return lad


@pytest.mark.parametrize("what", ["history", "evolving", "mixture", "everything"])
def test_shifted_counters_leave_the_chains_alone(what):
    kw = dict(history=dict(N=3, cap=64), evolving=dict(evolve=0.03), mixture=dict(mix=3), everything=dict(N=3, cap=64, evolve=0.03, mix=2))[what]
    young, aged = checker(**kw), checker(**kw)
    for lad in (young, aged):
        lad.pt_step(4)
    N, cap = kw.get("N", 1), kw.get("cap", 0)
    steps = 7
    d = AU.largest_shift(max(int(aged.ntries.max()), int(aged.nhist.max())), steps, N * cap if cap else 1)
    assert d % (N * max(cap, 1)) == 0 and d > 2**31 - 200 - N * max(cap, 1)
    rows_before = aged.nsize.copy()
    AU.age_checker(aged, aged.step, d)
    assert aged.step == young.step == 4
    for k in range(steps):
        (young.sweep if k == 3 else young.pt_step)(1)
        (aged.sweep if k == 3 else aged.pt_step)(1)
        for name in ("x", "llike", "lprior", "last_type", "nsize", "betaw", "swap_count", "swap_accept_count", "last_pairs", "last_accept"):
            assert np.array_equal(getattr(young, name), getattr(aged, name)), (name, k)
        for name in ("ntries", "naccept", "nhist"):
            assert np.array_equal(getattr(young, name) + d, getattr(aged, name)), (name, k)
    # the run ended as late as the ring's period lets it, and at least MARGIN below the limit
    assert AU.COUNT_MAX - AU.MARGIN - 2 * steps - N * max(cap, 1) < int(max(aged.nhist.max(), aged.ntries.max())) <= AU.COUNT_MAX - AU.MARGIN
    if cap:
        hy, ha = young.history(), aged.history()
        assert (aged.nsize > rows_before).all()          # rows were saved at the aged counters
        for name in ("x", "llike", "lprior", "last_type", "invtemp"):
            for c in range(young.N):
                n = int(young.nsize[c])
                assert np.array_equal(hy[name][c, :n], ha[name][c, :n]), (name, c)
        for name in ("ntries", "naccept"):
            for c in range(young.N):
                n0, n = int(rows_before[c]), int(young.nsize[c])
                assert np.array_equal(hy[name][c, :n0], ha[name][c, :n0]) and np.array_equal(hy[name][c, n0:n] + d, ha[name][c, n0:n]), (name, c)
    assert (young.naccept.sum() - young.N) > 0 and (young.ntries - young.naccept).sum() > 0 and young.swap_count.sum() > 0


@pytest.mark.parametrize("what", ["plain", "everything"])
def test_a_dropped_high_word_of_the_step_is_seen_at_once(what):
    """what a 32-bit copy of the step would do at 2^32: go on from step 0.  The chains part on the very next step."""
    kw = dict(plain={}, everything=dict(N=3, cap=64, evolve=0.03, mix=2))[what]
    whole, cut = checker(step=AU.LATE_STEP, **kw), checker(step=AU.LATE_STEP, **kw)
    for lad in (whole, cut):
        lad.pt_step(2)
    assert whole.step == cut.step == 2**32 and np.array_equal(whole.x, cut.x)
    cut.s.contents.step = whole.step & 0xFFFFFFFF
    assert cut.step == 0
    for k in range(3):
        whole.pt_step(1); cut.pt_step(1)
        frac = float(np.mean(whole.x != cut.x))
        print("step %d: %.2f of all coordinates differ" % (k, frac))
        assert frac >= 0.25, (k, frac)
    # and the other way round: the steps below 2^32 are not the steps 2^32 above them
    low, high = checker(step=1, **kw), checker(step=2**32 + 1, **kw)
    low.pt_step(1); high.pt_step(1)
    assert float(np.mean(low.x != high.x)) >= 0.25


def test_no_chain_makes_more_than_two_adds_in_a_step_and_some_make_two():
    """PTM_ADDS_PER_STEP: a rung in two exchange trials of one step (pair (r, r+1) picked before pair (r-1, r))"""
    lad = checker()
    worst = 0
    for _ in range(400):
        before_h, before_t = lad.nhist, lad.ntries
        lad.pt_step(1)
        dh, dt = lad.nhist - before_h, lad.ntries - before_t
        assert dh.min() >= 1 and dh.max() <= AU.ADDS_PER_STEP and dt.max() <= 1
        assert dt.min() >= 0 and (dh[dt == 1] == 1).all()   # a Metropolis move is one add; a rung in a trial makes no move
        worst = max(worst, int(dh.max()))
    assert worst == AU.ADDS_PER_STEP


# ---- the counter layout, against an independent restatement -----------------------------------------------------------------
M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al. 2011), restated from the paper: ten rounds, the key bumped by the Weyl constants between them"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return [c0, c1, c2, c3]


def draw_block(seed, tag, stream, step, block):
    """the engine's counter layout (ptm_device_math.hpp): c0 = block, c1 = stream, c2 = step[31:0], c3 = step[55:32] | tag << 24"""
    return philox4x32_10([block, stream, step & M32, ((step >> 32) & 0xFFFFFF) | (tag << 24)], [seed & M32, seed >> 32])


LATE_STEPS = (2**32 - 1, 2**32, 2**32 + 1, 2**40 + 5, 2**56 - 1)
TAGS = (0, 1, 2, 3, 4)   # TAG_MH, TAG_PT, TAG_INIT, TAG_SET, TAG_PRIOR


def test_the_restatement_gives_the_known_answers():
    # Random123 kat_vectors, philox4x32 10 rounds (the three tests/test_oracle_golden.py holds the checker to)
    assert philox4x32_10([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert philox4x32_10([M32] * 4, [M32] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert philox4x32_10([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_counter_layout_at_the_edges_of_the_step_words():
    rng = np.random.default_rng(17)
    seen = set()
    for step in LATE_STEPS + (0, 1, 2**31, 2**32 - 2):
        for tag in TAGS:
            for seed, stream, block in ((0, 0, 0), (SEED, 7, 3), (int(rng.integers(0, 2**63)) * 2 + 1, int(rng.integers(0, 2**32)), int(rng.integers(0, 300)))):
                got = O.draw_block(seed, tag, stream, step, block)
                assert got == draw_block(seed, tag, stream, step, block), (hex(seed), tag, stream, step, block)
                seen.add((seed, stream, block, tuple(got)))
    # every (step, tag) is a stream of its own: no two of them drew the same block
    assert len(seen) == 9 * 5 * 3
    # the high word and the tag share c3: step[55:32] does not run into the tag
    assert O.draw_block(1, 0, 0, 2**56 - 1, 0) != O.draw_block(1, 1, 0, 2**56 - 1, 0)
    assert O.draw_block(1, 0, 0, (2**24 - 1) << 32, 0) == draw_block(1, 0, 0, (2**24 - 1) << 32, 0) != draw_block(1, 255, 0, 0, 0)


# ---- the horizon's arithmetic -----------------------------------------------------------------------------------------------
def test_the_limit_is_one_constant():
    hdr = open(os.path.join(ROOT, "include", "ptm_engine.h")).read()
    assert int(re.search(r"#define PTM_COUNT_MAX (\d+)", hdr).group(1)) == E.COUNT_MAX == AU.COUNT_MAX == 2**31 - 1
    lim = open(os.path.join(CSRC, "ptm_count_limit.hpp")).read()
    assert int(re.search(r"PTM_ADDS_PER_STEP = (\d+);", lim).group(1)) == AU.ADDS_PER_STEP
    assert "hip" not in lim.lower().replace("no hip", "")     # plain C++: a stand-alone program reads it


def test_largest_shift_is_the_largest():
    for top, steps, unit in ((1, 7, 1), (29, 7, 192), (40, 10, 64), (3, 1, 2**24 * 120), (1000, 0, 3 * 64)):
        d = AU.largest_shift(top, steps, unit)
        assert d % unit == 0 and d > 0
        assert top + d + AU.ADDS_PER_STEP * steps <= AU.COUNT_MAX - AU.MARGIN < top + d + unit + AU.ADDS_PER_STEP * steps


def test_guard_arithmetic_under_the_sanitizers():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "count_limit")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-I", CSRC,
                               os.path.join(ROOT, "tests", "cxx", "count_limit_main.cc"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"checks=(\d+)\n", r.stdout)
    assert m and int(m.group(1)) > 1000, r.stdout
