"""Split R-hat across a population's walkers on the device (ptm_rhat, ptm_rhat_series): the kernels of
ptmcmc_amd/csrc/ptm_rhat_kernels.hpp restate the facade's rhat_estimator with one lane per (walker, half, feature) and then one per
feature, every sum in the host's order -- so their answers must carry the host estimator's very bits (tests/rhat_model.py is its
line-by-line Python twin, pinned to the facade by tests/test_rhat_model_cpu.py)."""
import numpy as np
import pytest

import rhat_model as R
from ptmcmc_amd import engine as E
from ptmcmc_amd.problems import GaussianProblem

pytestmark = pytest.mark.gpu

NAMES = ("rhat", "mean", "within", "between", "seq_mean", "seq_var")


def same_bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def assert_same(got, want, what):
    assert len(got) == len(want) == 6
    for name, g, w in zip(NAMES, got, want):
        assert np.shape(g) == np.shape(w) and same_bits(g, w), (what, name, np.ravel(g)[:4], np.ravel(w)[:4])


# ---- a caller's series ------------------------------------------------------------------------------------------------------
N_S, NS_S, NF_S = 600, 70, 3


def ar1_series(n, ns, nf, seed):
    rng = np.random.default_rng(seed)
    phi = rng.uniform(0.2, 0.95, size=(ns, nf))
    e = rng.standard_normal((n, ns, nf))
    x = np.empty_like(e)
    cur = np.zeros((ns, nf))
    for t in range(n):
        cur = phi * cur + e[t]
        x[t] = cur
    return x + np.arange(nf) * 7.0


@pytest.fixture(scope="module")
def series():
    return ar1_series(N_S, NS_S, NF_S, 1)


@pytest.mark.parametrize("nrows", [4, 250, 600])
def test_series_of_a_ragged_last_wave_equal_the_model(series, nrows):
    assert (2 * NS_S * NF_S) % 64                                   # the last wave is not full
    want = R.split_rhat(R.series_window(series, nrows), detail=True)
    assert np.isfinite(want[0]).all()
    assert_same(E.rhat_series(series, nrows, sequences=True), want, nrows)
    short = E.rhat_series(series, nrows)
    assert len(short) == 4 and all(same_bits(g, w) for g, w in zip(short, want))


def test_one_series_and_the_default_window(series):
    one = series[:, 3:4, :]
    assert_same(E.rhat_series(one, 250, sequences=True), R.split_rhat(R.series_window(one, 250), detail=True), "one series")
    odd = series[:N_S - 1]                                          # 599 rows: the default is the newest 598
    assert_same(E.rhat_series(odd, sequences=True), R.split_rhat(R.series_window(odd, N_S - 2), detail=True), "default nrows")


def test_exact_cases():
    x = R.equal_sequences()
    rhat, mean, within, between = E.rhat_series(x)
    assert (between == 0).all() and (mean == 3).all() and within.tolist() == [2.0, 8.0]
    assert same_bits(rhat, np.full(2, np.sqrt(4.0 / 5.0)))
    x = R.two_groups()
    got = E.rhat_series(x, sequences=True)
    assert_same(got, R.split_rhat(x, detail=True), "two groups")
    assert (got[0] > 2).all() and (np.abs(got[0] - 5.0) < 0.5).all()
    x = ar1_series(20, 3, 2, 5)
    x[:, :, 1] = 2.5                                                # a constant feature: the formula's 0 / 0
    got = E.rhat_series(x, sequences=True)
    assert_same(got, R.split_rhat(x, detail=True), "constant feature")
    assert np.isfinite(got[0][0]) and np.isnan(got[0][1])


def test_series_refusals(series):
    for nrows in (3, 2, 0, 5, N_S + 2):
        with pytest.raises(E.PtmError):
            E.rhat_series(series, nrows)
    out = tuple(np.full(NF_S, -7.0) for _ in range(4))
    with pytest.raises(E.PtmError):
        E.rhat_series(series, N_S + 2, out=out)
    assert all((o == -7.0).all() for o in out)


# ---- the engine's history ring --------------------------------------------------------------------------------------------------
DIM, NT, W, ADD, HR, STEPS = 3, 4, 70, 2, 2, 3000


def run_engine(capacity, dim=DIM, nt=NT, steps=STEPS, add=ADD, hr=HR, swap_rate=0.1, seed=0x5EED0E57):
    pr = GaussianProblem(dim, nt, 1e2)
    eng = E.Engine(dim, nt, W, seed=seed, swap_rate=swap_rate, add_every_n=add, history_rungs=hr, history_capacity=capacity)
    pr.configure(eng, E.PROP_LOWER)
    eng.init_from_prior()
    eng.step(steps)
    eng.sync()
    return eng


def ring_want(hist, nh, rung, nfeat, nrows, add=ADD):
    ok, win = R.ring_window(hist, slice(rung * W, (rung + 1) * W), add, nh[rung], nrows)
    assert ok
    return R.split_rhat(win[:, :, :nfeat], detail=True), win


@pytest.fixture(scope="module")
def ring():
    eng = run_engine(1 + STEPS // ADD + 99)
    hist = eng.history()
    nh = eng.nhist.reshape(NT, W)
    assert (nh[:HR] == STEPS).all()
    yield eng, hist, nh
    eng.close()


@pytest.mark.parametrize("rung,nfeat", [(0, 3), (1, 3), (0, 2), (1, 2)])
def test_engine_ring_equals_the_model_and_the_series_call(ring, rung, nfeat):
    eng, hist, nh = ring
    _, rows = ring_want(hist, nh, rung, DIM, STEPS // ADD)         # every saved row behind the start state
    for nrows in (4, 500, 1500):
        want, _ = ring_want(hist, nh, rung, nfeat, nrows)
        got = eng.split_rhat(rung, nfeat, nrows, sequences=True)
        assert_same(got, want, (rung, nfeat, nrows))
        assert_same(E.rhat_series(rows[:, :, :nfeat], nrows, sequences=True), got, ("series", rung, nfeat, nrows))
        assert np.isfinite(got[0]).all() and (got[0] > 0.7).all()
    # the default: all features, the largest even window every walker still has
    if nfeat == DIM:
        assert_same(eng.split_rhat(rung, sequences=True), ring_want(hist, nh, rung, DIM, 1500)[0], "default window")


@pytest.mark.parametrize("nfeat", [20, 5])
def test_ring_in_the_permuted_layout_of_32_dimensions(nfeat):
    dim, steps = 20, 300
    eng = run_engine(steps + 20, dim=dim, nt=2, steps=steps, add=1, hr=1)
    try:
        hist, nh = eng.history(), eng.nhist.reshape(2, W)
        assert (nh[0] == steps).all()
        for nrows in (4, 150, 300):
            ok, win = R.ring_window(hist, slice(0, W), 1, nh[0], nrows)
            assert ok
            got = eng.split_rhat(0, nfeat, nrows, sequences=True)
            assert_same(got, R.split_rhat(win[:, :, :nfeat], detail=True), (nfeat, nrows))
            # the features are told apart: the sequence means of no two of them coincide
            assert len({v.tobytes() for v in got[4].T}) == nfeat
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
        print("rung 1 add_state counts", sorted(set(counts.tolist())))
        assert counts.min() >= steps and len(set(counts.tolist())) >= 3
        assert len(set((1 + (counts - 1) // ADD).tolist())) >= 2   # ... and in their newest rows
        for rung in (0, 1):
            for nfeat, nrows in ((3, 1000), (2, 4), (3, 1500)):
                want, _ = ring_want(hist, nh, rung, nfeat, nrows)
                assert_same(eng.split_rhat(rung, nfeat, nrows, sequences=True), want, (rung, nfeat, nrows))
    finally:
        eng.close()


def test_wrapped_ring():
    cap = 1300
    eng = run_engine(cap)
    try:
        hist, nh = eng.history(), eng.nhist.reshape(NT, W)
        assert hist["row"].max() == STEPS // ADD and hist["row"][hist["row"] >= 0].min() > 1     # slots have wrapped
        for rung, nfeat, nrows in ((0, 3, 1000), (1, 2, 1300), (1, 3, 4)):                       # windows the ring still holds
            want, _ = ring_want(hist, nh, rung, nfeat, nrows)
            assert_same(eng.split_rhat(rung, nfeat, nrows, sequences=True), want, (rung, nfeat, nrows))
        assert_same(eng.split_rhat(0, sequences=True), ring_want(hist, nh, 0, DIM, cap)[0], "default window")
        # a window that reaches a row the ring has lost: refused, and the caller's arrays stay as they were
        assert not R.ring_window(hist, slice(0, W), ADD, nh[0], cap + 2)[0]
        out = tuple(np.full(DIM, -7.0) for _ in range(4)) + tuple(np.full((2 * W, DIM), -7.0) for _ in range(2))
        with pytest.raises(E.PtmError) as ei:
            eng.split_rhat(0, DIM, cap + 2, sequences=True, out=out)
        assert "history_capacity must hold the window" in str(ei.value)
        assert all((o == -7.0).all() for o in out)
    finally:
        eng.close()


def test_aged_ring_row_numbers_near_the_estimators_limit_and_the_refusal_beyond_it():
    """the chains' add_state counts just below 2e9 (tests/aging_util.py): saved row numbers of 6.6e8 in a wrapped ring give the bits
    of the young twin, whose rows are the same but for the shift; past 2e9 adds the call refuses and leaves its outputs alone"""
    import aging_util as AU
    import history_readers_util as HU
    D, Nt, add, steps, cap, limit = 2, 6, 3, 300, 75, 2000000000
    make = lambda: HU.make_engine(D, Nt, W, "lower", add, 0xE71D7, 0.4, Nt, cap, 0.01)
    young, aged = make(), make()
    try:
        for e in (young, aged):
            e.step(steps); e.sync()
        unit = add * cap
        AU.age_engine(aged, young.step_count, (limit - AU.MARGIN - int(aged.nhist.max())) // unit * unit, add)
        nh = aged.nhist.reshape(Nt, W)
        assert limit - AU.MARGIN - unit < nh.max() <= limit - AU.MARGIN and len(set(nh[1].tolist())) > 1
        hist = aged.history()
        assert hist["row"].max() >= cap                                 # a wrapped ring of late rows
        for rung, nfeat, nrows in ((0, 2, 74), (1, 2, 74), (3, 1, 4)):
            ok, win = R.ring_window(hist, slice(rung * W, (rung + 1) * W), add, nh[rung], nrows)
            assert ok
            got = aged.split_rhat(rung, nfeat, nrows, sequences=True)
            assert_same(got, R.split_rhat(win[:, :, :nfeat], detail=True), ("aged", rung, nfeat, nrows))
            assert_same(got, young.split_rhat(rung, nfeat, nrows, sequences=True), ("young twin", rung, nfeat, nrows))
        AU.age_engine(aged, young.step_count, (AU.COUNT_MAX - AU.MARGIN - int(aged.nhist.max())) // unit * unit, add)
        assert limit < aged.nhist.max()
        out = tuple(np.full(D, -7.0) for _ in range(4))
        with pytest.raises(E.PtmError) as err:
            aged.split_rhat(1, D, 74, out=out)
        assert str(err.value).startswith("ptm error -2:") and "more than 2e9 steps" in str(err.value)
        assert all((o == -7.0).all() for o in out)
    finally:
        young.close(); aged.close()


def test_refusals(ring):
    eng, _, _ = ring
    assert np.isfinite(eng.split_rhat(0, DIM, 500)[0]).all()
    for rung, nfeat, nrows in ((0, DIM, 501), (0, DIM, 2), (0, 0, 500), (0, DIM + 1, 500), (HR, DIM, 500), (0, DIM, STEPS // ADD + 2), (-1, DIM, 500)):
        with pytest.raises(E.PtmError):
            eng.split_rhat(rung, nfeat, nrows)
    with pytest.raises(E.PtmError):
        eng.split_rhat(HR)                                          # (also with the default window)
    with eng.batch():
        with pytest.raises(E.PtmError):
            eng.split_rhat(0, DIM, 500)                             # between batch_begin and batch_end
    plain = E.Engine(DIM, NT, 4)
    try:
        with pytest.raises(E.PtmError):
            plain.split_rhat(0, DIM, 4)                             # no history ring
    finally:
        plain.close()
    assert np.isfinite(eng.split_rhat(0, DIM, 500)[0]).all()        # the engine is none the worse for it
