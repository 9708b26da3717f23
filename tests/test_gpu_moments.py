"""Pooled posterior mean and covariance of a rung on the device (ptm_moments, ptm_moments_series): the kernels of
ptmcmc_amd/csrc/ptm_moments_kernels.hpp restate the facade's moments_estimator -- sums over a walker's rows, over the 64 walkers of a
block, over the blocks, every one sequential -- so their answers must carry the host estimator's very bits (tests/moments_model.py
is its Python twin, pinned to the facade by tests/test_moments_model_cpu.py)."""
import numpy as np
import pytest

import moments_model as M
import rhat_model as R
from ptmcmc_amd import engine as E
from ptmcmc_amd.problems import GaussianProblem

pytestmark = pytest.mark.gpu

NAMES = ("mean", "cov", "var", "walker_sum", "count")


def same_bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def assert_same(got, want, what):
    assert len(got) == len(want) == 5
    for name, g, w in zip(NAMES, got, want):
        if g is None or w is None:
            assert g is None and w is None, (what, name)
        else:
            assert np.shape(g) == np.shape(w) and same_bits(g, w), (what, name, np.ravel(g)[:4], np.ravel(w)[:4])


def series_case(series, nrows, what, cov=True):
    want = M.moments(M.series_window(series, nrows), cov=cov)
    assert np.isfinite(want[0]).all() and np.isfinite(want[2]).all()
    assert_same(E.moments_series(series, nrows, cov=cov, walker_sums=True), want, what)
    return want


# ---- a caller's series ------------------------------------------------------------------------------------------------------
NS_S, NF_S = 70, 3
TILE_S = 4096 // NF_S


@pytest.fixture(scope="module")
def series():
    return M.ar1_series(TILE_S + 40, NS_S, NF_S, 1)


@pytest.mark.parametrize("nrows", [1, 2, 5, 250, TILE_S, TILE_S + 1])
def test_series_of_a_ragged_last_wave_and_a_second_block_of_six_equal_the_model(series, nrows):
    assert (NS_S * NF_S) % 64 and NS_S - 64 == 6 and E.moments_tile_rows(NF_S) == TILE_S
    want = series_case(series, nrows, nrows)
    short = E.moments_series(series, nrows)
    assert len(short) == 4 and all(same_bits(g, w) for g, w in zip(short, want[:3])) and short[3] == NS_S * nrows
    only_var = E.moments_series(series, nrows, cov=False)            # the variances alone: the other kernel, the same bits
    assert only_var[1] is None and same_bits(only_var[0], want[0]) and same_bits(only_var[2], want[2])


@pytest.mark.parametrize("ns", [1, 64, 65, 129])
def test_series_counts_around_the_block_of_64(ns):
    x = M.ar1_series(9, ns, 3, 10 + ns)
    for nrows in (2, 9):
        series_case(x, nrows, (ns, nrows))
    assert_same(E.moments_series(x, walker_sums=True), M.moments(x), (ns, "default window"))


def test_walkers_taken_a_group_at_a_time_give_the_same_bits(monkeypatch):
    x = M.ar1_series(7, 129, 5, 3)
    want = M.moments(x)
    monkeypatch.setenv("PTM_MOMENTS_GROUP", "64")                   # three launches of the cross kernel: 64, 64 and 1 walkers
    assert_same(E.moments_series(x, walker_sums=True), want, "groups of 64")
    monkeypatch.setenv("PTM_MOMENTS_GROUP", "100")                  # rounded down to whole blocks
    assert_same(E.moments_series(x, walker_sums=True), want, "groups of 100")


@pytest.mark.parametrize("nf,ns,rows", [(24, 65, (3,)), (33, 70, (5, 4096 // 33 + 1)), (128, 3, (2, 4096 // 128 + 1)), (128, 65, (3,)), (127, 2, (33,))])
def test_many_pairs(nf, ns, rows):
    """more pairs than a workgroup has lanes.  24 features: 300 pairs, two a lane; 33: 561 pairs, three a lane (lanes with two and
    with three of their own); 128: 8256 pairs, four a lane in nine chunks of pairs per walker"""
    assert E.moments_tile_rows(nf) == 4096 // nf
    x = M.ar1_series(max(rows), ns, nf, nf + ns)
    for nrows in rows:
        want = series_case(x, nrows, (nf, ns, nrows))
        assert same_bits(want[1], want[1].T) and len({v.tobytes() for v in want[1]}) == nf     # the features are told apart


def test_above_128_features_the_variances_are_served_and_the_covariance_is_refused():
    x = M.ar1_series(6, 5, 130, 2)
    series_case(x, 6, "130 features", cov=False)
    out = (np.full(130, -7.0), np.full((130, 130), -7.0), np.full(130, -7.0))
    with pytest.raises(E.PtmError) as ei:
        E.moments_series(x, 6, out=out)
    assert str(ei.value).startswith("ptm error -2:") and all((o == -7.0).all() for o in out)


def test_a_constant_feature_gives_exact_zeros():
    x = M.ar1_series(20, 65, 3, 5)
    x[:, :, 1] = 2.5
    mean, cov, var, n = E.moments_series(x)
    assert mean[1] == 2.5 and (cov[1] == 0).all() and (cov[:, 1] == 0).all() and var[1] == 0 and n == 20 * 65
    assert cov[0, 0] > 0 and cov[2, 2] > 0
    assert_same(E.moments_series(x, walker_sums=True), M.moments(x), "constant feature")


def test_series_refusals(series):
    n = series.shape[0]
    for nrows in (0, -1, n + 1):
        with pytest.raises(E.PtmError):
            E.moments_series(series, nrows)
    out = (np.full(NF_S, -7.0), np.full((NF_S, NF_S), -7.0), np.full(NF_S, -7.0), np.full((NS_S, NF_S), -7.0))
    with pytest.raises(E.PtmError):
        E.moments_series(series, n + 1, walker_sums=True, out=out)
    one = (np.full(NF_S, -7.0), np.full((NF_S, NF_S), -7.0), np.full(NF_S, -7.0))
    with pytest.raises(E.PtmError):
        E.moments_series(series[:, :1], 1, out=one)                # N = 1
    assert all((o == -7.0).all() for o in out + one)


# ---- the engine's history ring --------------------------------------------------------------------------------------------------
DIM, NT, W, ADD, HR, STEPS = 3, 4, 70, 2, 2, 3000


def run_engine(capacity, dim=DIM, nt=NT, steps=STEPS, add=ADD, hr=HR, swap_rate=0.1, seed=0x5EED0E57, walkers=W):
    pr = GaussianProblem(dim, nt, 1e2)
    eng = E.Engine(dim, nt, walkers, seed=seed, swap_rate=swap_rate, add_every_n=add, history_rungs=hr, history_capacity=capacity)
    pr.configure(eng, E.PROP_LOWER)
    eng.init_from_prior()
    eng.step(steps)
    eng.sync()
    return eng


def ring_want(hist, nh, rung, nfeat, nrows, add=ADD, walkers=W):
    ok, win = R.ring_window(hist, slice(rung * walkers, (rung + 1) * walkers), add, nh[rung], nrows)
    assert ok
    return M.moments(win[:, :, :nfeat]), win


@pytest.fixture(scope="module")
def ring():
    eng = run_engine(1 + STEPS // ADD + 99)
    hist = eng.history()
    nh = eng.nhist.reshape(NT, W)
    assert (nh[:HR] == STEPS).all()
    yield eng, hist, nh
    eng.close()


@pytest.mark.parametrize("rung,nfeat", [(0, 3), (1, 3), (0, 2), (1, 1)])
def test_engine_ring_equals_the_model_and_the_series_call(ring, rung, nfeat):
    eng, hist, nh = ring
    _, rows = ring_want(hist, nh, rung, DIM, STEPS // ADD)         # every saved row behind the start state
    for nrows in (1, 5, 1500):
        want, _ = ring_want(hist, nh, rung, nfeat, nrows)
        got = eng.posterior_moments(rung, nfeat, nrows, walker_sums=True)
        assert_same(got, want, (rung, nfeat, nrows))
        assert_same(E.moments_series(rows[:, :, :nfeat], nrows, walker_sums=True), got, ("series", rung, nfeat, nrows))
        assert np.isfinite(got[1]).all() and (got[2] > 0).all()
    if nfeat == DIM:                                                # the default: all features, every row every walker still has
        assert_same(eng.posterior_moments(rung, walker_sums=True), ring_want(hist, nh, rung, DIM, 1500)[0], "default window")
        mean, cov, var, n = eng.posterior_moments(rung)
        assert n == W * 1500 and same_bits(var, np.diagonal(cov))
        only_var = eng.posterior_moments(rung, cov=False)
        assert only_var[1] is None and same_bits(only_var[2], var) and same_bits(only_var[0], mean)


@pytest.mark.parametrize("nfeat", [20, 5])
def test_ring_in_the_permuted_layout_of_32_dimensions(nfeat):
    dim, steps = 20, 300
    eng = run_engine(steps + 20, dim=dim, nt=2, steps=steps, add=1, hr=1)
    try:
        hist, nh = eng.history(), eng.nhist.reshape(2, W)
        assert (nh[0] == steps).all()
        for nrows in (1, 150, 300):
            ok, win = R.ring_window(hist, slice(0, W), 1, nh[0], nrows)
            assert ok
            got = eng.posterior_moments(0, nfeat, nrows, walker_sums=True)
            assert_same(got, M.moments(win[:, :, :nfeat]), (nfeat, nrows))
            assert len({v.tobytes() for v in got[1]}) == nfeat      # the features are told apart
    finally:
        eng.close()


def test_walkers_with_different_add_state_counts_each_use_their_own_window():
    """five exchange candidates per step: a rung exchanged twice in a step makes an extra add_state call, so the walkers of rung 1
    differ in their counts, and with them in their newest saved row"""
    nt, steps = 8, 3000
    eng = run_engine(1 + steps // ADD + 1500, nt=nt, steps=steps, swap_rate=0.3, seed=0x5EED0E56)
    try:
        assert eng.max_swaps == 5
        hist, nh = eng.history(), eng.nhist.reshape(nt, W)
        counts = nh[1]
        assert counts.min() >= steps and len(set(counts.tolist())) >= 3
        assert len(set((1 + (counts - 1) // ADD).tolist())) >= 2   # ... and in their newest rows
        for rung in (0, 1):
            for nfeat, nrows in ((3, 1000), (2, 1), (3, 1500)):
                want, _ = ring_want(hist, nh, rung, nfeat, nrows)
                assert_same(eng.posterior_moments(rung, nfeat, nrows, walker_sums=True), want, (rung, nfeat, nrows))
    finally:
        eng.close()


def test_wrapped_ring():
    cap = 1300
    eng = run_engine(cap)
    try:
        hist, nh = eng.history(), eng.nhist.reshape(NT, W)
        assert hist["row"].max() == STEPS // ADD and hist["row"][hist["row"] >= 0].min() > 1     # slots have wrapped
        for rung, nfeat, nrows in ((0, 3, 1000), (1, 2, 1300), (1, 3, 1)):                       # windows the ring still holds
            want, _ = ring_want(hist, nh, rung, nfeat, nrows)
            assert_same(eng.posterior_moments(rung, nfeat, nrows, walker_sums=True), want, (rung, nfeat, nrows))
            only_var = eng.posterior_moments(rung, nfeat, nrows, cov=False)
            assert same_bits(only_var[2], want[2])
        assert_same(eng.posterior_moments(0, walker_sums=True), ring_want(hist, nh, 0, DIM, cap)[0], "default window")
        # a window that reaches a row the ring has lost: refused, and the caller's arrays stay as they were
        assert not R.ring_window(hist, slice(0, W), ADD, nh[0], cap + 2)[0]
        for cov in (True, False):
            out = (np.full(DIM, -7.0), np.full((DIM, DIM), -7.0) if cov else None, np.full(DIM, -7.0), np.full((W, DIM), -7.0))
            with pytest.raises(E.PtmError) as ei:
                eng.posterior_moments(0, DIM, cap + 2, walker_sums=True, out=out)
            assert "history_capacity must hold the window" in str(ei.value)
            assert all((o == -7.0).all() for o in out if o is not None)
    finally:
        eng.close()


def test_ragged_counts_in_a_wrapped_ring():
    """walkers that differ in their counts, in a ring that has wrapped: every walker's own newest `capacity` rows are there and make
    the largest window; one row more is refused"""
    nt, steps, cap = 8, 3000, 1000
    eng = run_engine(cap, nt=nt, steps=steps, swap_rate=0.3, seed=0x5EED0E56)
    try:
        hist, nh = eng.history(), eng.nhist.reshape(nt, W)
        assert len(set(nh[1].tolist())) >= 3
        want, _ = ring_want(hist, nh, 1, DIM, cap)
        assert_same(eng.posterior_moments(1, DIM, cap, walker_sums=True), want, "a full ring")
        out = (np.full(DIM, -7.0), np.full((DIM, DIM), -7.0), np.full(DIM, -7.0))
        with pytest.raises(E.PtmError):
            eng.posterior_moments(1, DIM, cap + 1, out=out)
        assert all((o == -7.0).all() for o in out)
    finally:
        eng.close()


def test_chains_past_2e9_adds_are_refused():
    import aging_util as AU
    import history_readers_util as HU
    D, Nt, add, steps, cap = 2, 6, 3, 300, 75
    make = lambda: HU.make_engine(D, Nt, W, "lower", add, 0xE71D7, 0.4, Nt, cap, 0.01)
    young, aged = make(), make()
    try:
        for e in (young, aged):
            e.step(steps); e.sync()
        unit = add * cap
        AU.age_engine(aged, young.step_count, (2000000000 - AU.MARGIN - int(aged.nhist.max())) // unit * unit, add)
        nh = aged.nhist.reshape(Nt, W)
        hist = aged.history()
        assert hist["row"].max() >= cap                                 # a wrapped ring of late rows
        for rung, nfeat, nrows in ((0, 2, 74), (1, 2, 74), (3, 1, 1)):
            ok, win = R.ring_window(hist, slice(rung * W, (rung + 1) * W), add, nh[rung], nrows)
            assert ok
            got = aged.posterior_moments(rung, nfeat, nrows, walker_sums=True)
            assert_same(got, M.moments(win[:, :, :nfeat]), ("aged", rung, nfeat, nrows))
            assert_same(got, young.posterior_moments(rung, nfeat, nrows, walker_sums=True), ("young twin", rung, nfeat, nrows))
        AU.age_engine(aged, young.step_count, (AU.COUNT_MAX - AU.MARGIN - int(aged.nhist.max())) // unit * unit, add)
        assert 2000000000 < aged.nhist.max()
        out = (np.full(D, -7.0), np.full((D, D), -7.0), np.full(D, -7.0))
        with pytest.raises(E.PtmError) as err:
            aged.posterior_moments(1, D, 74, out=out)
        assert str(err.value).startswith("ptm error -2:") and "more than 2e9 steps" in str(err.value)
        assert all((o == -7.0).all() for o in out)
    finally:
        young.close(); aged.close()


def test_refusals(ring):
    eng, _, _ = ring
    assert np.isfinite(eng.posterior_moments(0, DIM, 500)[1]).all()
    out = (np.full(DIM, -7.0), np.full((DIM, DIM), -7.0), np.full(DIM, -7.0))
    for rung, nfeat, nrows in ((0, DIM, 0), (0, DIM, -2), (0, 0, 500), (0, DIM + 1, 500), (HR, DIM, 500), (0, DIM, STEPS // ADD + 1), (-1, DIM, 500)):
        with pytest.raises(E.PtmError):
            eng.posterior_moments(rung, nfeat, nrows, out=out)
    with pytest.raises(E.PtmError):
        eng.posterior_moments(HR)                                   # (also with the default window)
    with eng.batch():
        with pytest.raises(E.PtmError):
            eng.posterior_moments(0, DIM, 500, out=out)             # between batch_begin and batch_end
    assert all((o == -7.0).all() for o in out)
    plain = E.Engine(DIM, NT, 4)
    try:
        with pytest.raises(E.PtmError):
            plain.posterior_moments(0, DIM, 4)                      # no history ring
    finally:
        plain.close()
    lone = run_engine(20, steps=10, walkers=1)                      # one walker: one row is one sample
    try:
        with pytest.raises(E.PtmError):
            lone.posterior_moments(0, DIM, 1, out=out)
        assert all((o == -7.0).all() for o in out)
        _, rows = ring_want(lone.history(), lone.nhist.reshape(NT, 1), 0, DIM, 5, walkers=1)
        assert_same(lone.posterior_moments(0, DIM, 5, walker_sums=True), M.moments(rows), "one walker")
    finally:
        lone.close()
    assert np.isfinite(eng.posterior_moments(0, DIM, 500)[1]).all()   # the engine is none the worse for it
