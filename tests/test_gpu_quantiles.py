"""Exact posterior quantiles of a rung on the device (ptm_quantiles, ptm_quantiles_series): the kernels of
ptmcmc_amd/csrc/ptm_quantiles_kernels.hpp select the order statistics the facade's quantile_estimator sorts for, so their answers
-- q and the bracket x_lo, x_hi -- must carry the host estimator's very bits (tests/quantiles_model.py is its Python twin, pinned to
the facade by tests/test_quantiles_model_cpu.py), on every path the environment can force: every pass over the ring, the candidates
packed into the workspace, and a packed path whose room is too small so that it falls back to the ring."""
import numpy as np
import pytest

import quantiles_model as Q
import rhat_model as R
from ptmcmc_amd import engine as E
from ptmcmc_amd.problems import GaussianProblem

pytestmark = pytest.mark.gpu

NAMES = ("q", "x_lo", "x_hi", "count")
PATHS = {
    "default": {},
    "ring": {"PTM_QUANTILES_PATH": "ring"},
    "packed": {"PTM_QUANTILES_PATH": "packed"},
    "overflow": {"PTM_QUANTILES_PATH": "packed", "PTM_QUANTILES_PACK_BYTES": "64"},     # room for 64 / (8 nfeat) candidates a feature
    "tile of one": {"PTM_QUANTILES_PATH": "packed", "PTM_QUANTILES_TILE": "1"},
    "tile of two, ring": {"PTM_QUANTILES_PATH": "ring", "PTM_QUANTILES_TILE": "2"},
}
PROBS = [0.05, 0.5, 0.95]


def same_bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def assert_same(got, want, what):
    assert len(got) == len(want) == 4
    for name, g, w in zip(NAMES, got, want):
        assert np.shape(g) == np.shape(w) and same_bits(g, w), (what, name, np.ravel(g)[:4], np.ravel(w)[:4])


@pytest.fixture(params=list(PATHS))
def path(request, monkeypatch):
    for name in ("PTM_QUANTILES_PATH", "PTM_QUANTILES_PACK_BYTES", "PTM_QUANTILES_TILE"):
        monkeypatch.delenv(name, raising=False)
    for name, value in PATHS[request.param].items():
        monkeypatch.setenv(name, value)
    return request.param


def check_path(path, N=0):
    """the call that just ran took the path that was forced"""
    packed, ring_passes, packed_passes = E.quantiles_last_path()
    assert packed == (packed_passes > 0)
    if "ring" in path or path == "default":
        assert not packed
    return packed, ring_passes, packed_passes


def series_case(series, nrows, probs, what, path):
    want = Q.quantiles(Q.series_window(series, nrows), probs)
    assert_same(E.quantiles_series(series, probs, nrows, brackets=True), want, (what, path))
    check_path(path)
    return want


# ---- a caller's series ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [1, 64, 65, 129])
def test_series_shapes(ns, path):
    x = Q.skewed_series(257, ns, 3, 10 + ns)
    for nrows in (1, 2, 5, 257):
        want = series_case(x, nrows, PROBS, (ns, nrows), path)
        assert want[3] == ns * nrows
        if ns * nrows >= 640 and path == "packed":
            assert E.quantiles_last_path()[0]                       # the candidates behind the first digit were packed
        if ns * nrows >= 640 and path == "overflow":
            assert E.quantiles_last_path()[1] >= 2                  # ... or did not fit: the second pass walked the ring again
    short = E.quantiles_series(x, PROBS)                            # the default window, no brackets
    assert len(short) == 2 and same_bits(short[0], Q.quantiles(x, PROBS)[0]) and short[1] == 257 * ns


@pytest.mark.parametrize("nf", [1, 3, 33, 128])
def test_feature_counts_around_the_lds_tile(nf, path):
    """three probabilities: five or six slots, 21 features a tile; 32 probabilities: up to 64 slots, two features a tile"""
    x = Q.skewed_series(5, 65, nf, nf)
    want = series_case(x, 5, PROBS, nf, path)
    assert len({v.tobytes() for v in want[0].T}) == nf              # the features are told apart
    rng = np.random.default_rng(nf)
    many = np.concatenate([rng.uniform(0, 1, 26), [0.5, 0.5, 0.0, 1.0, 0.25, 0.25]])
    assert many.size == 32
    series_case(x, 5, many, (nf, "32 probabilities, repeats, unsorted"), path)


def test_a_single_sample(path):
    x = np.array([[[3.25, -0.0, -np.inf]]])
    want = series_case(x, 1, [0.0, 0.3, 1.0], "N = 1", path)
    assert same_bits(want[0], np.tile(x[0, 0], (3, 1)))


@pytest.mark.parametrize("N", [64, 65])
def test_probabilities(N, path):
    x = Q.skewed_series(1, N, 2, N)
    for probs in ([0.0, 1.0, 0.5], [1.0 / (N - 1), 7.0 / (N - 1), 0.25 if N == 65 else 1.0], [1e-12], [0.999999999999], [0.5]):
        want = series_case(x, 1, probs, (N, probs), path)
        assert (want[1] <= want[0]).all() and (want[0] <= want[2]).all()
    lo, hi, g = Q.ranks(65, 0.25)
    assert g == 0 and lo == 16                                      # a p with an integer h: q is the order statistic itself
    s = np.sort(x[0, :, 0])
    q, xlo, xhi, n = E.quantiles_series(x, [0.0, 1.0, 0.5], brackets=True)
    mid = Q.ranks(N, 0.5)                                           # (N odd: h is an integer, the bracket is still s_lo, s_lo+1)
    assert mid[:2] == ((N - 1) // 2, (N - 1) // 2 + 1)
    assert q[0, 0] == s[0] and q[1, 0] == s[-1] and xlo[2, 0] == s[mid[0]] and xhi[2, 0] == s[mid[1]] and n == N
    assert q[2, 0] == (s[32] if N == 65 else s[31] + 0.5 * (s[32] - s[31]))


def adversarial_features(N, seed):
    """[N, features]: the places a digit pass or a rank update goes wrong"""
    rng = np.random.default_rng(seed)
    f = []
    f.append(np.full(N, 2.5))                                                       # a constant feature
    three = np.repeat([-1.5, 2.0, 2.0000000000000004], [N // 3, N // 3, N - 2 * (N // 3)])
    f.append(rng.permutation(three))                                                # three values, ranks on the boundaries
    f.append(1.0 + rng.integers(0, 2, N) * 2.0 ** -52)                              # the lowest mantissa bit alone
    f.append(np.where(rng.integers(0, 2, N) == 1, 3.75, -3.75))                     # the sign alone
    f.append(np.where(rng.integers(0, 2, N) == 1, 0.0, -0.0))                       # zeros of both signs
    odd = np.array([1e-300, -1e300, 5e-324, -5e-324, 2.2e-308, np.inf, -np.inf, 0.0, -0.0, 1.0])
    f.append(odd[rng.integers(0, odd.size, N)])                                     # far-apart exponents, denormals, infinities
    f.append(-np.exp(rng.standard_normal(N)))                                       # all negative
    f.append(np.sort(rng.standard_normal(N)))                                       # already sorted
    f.append(np.sort(rng.standard_normal(N))[::-1])                                 # reversed
    f.append(np.full(N, -0.0))                                                      # a constant -0
    return np.stack(f, axis=1)


@pytest.mark.parametrize("ns,nrows", [(66, 1), (65, 9), (3, 700)])
def test_adversarial_values(ns, nrows, path):
    N = ns * nrows
    x = adversarial_features(N, N).reshape(nrows, ns, -1)
    third = N // 3
    probs = [0.0, 1.0, 0.5, (third - 1.0) / (N - 1), (third - 0.5) / (N - 1), third / (N - 1.0), (2 * third - 0.5) / (N - 1), 0.05, 0.95, 1e-12]
    want = series_case(x, nrows, probs, (ns, nrows), path)
    assert same_bits(want[0][:, 0], np.full(len(probs), 2.5))
    # a constant -0: the order statistics are -0; between two of them the formula gives -0 + g * (+0) = +0: nothing is special-cased
    assert same_bits(want[1][:, 9], np.full(len(probs), -0.0)) and same_bits(want[2][:, 9], want[1][:, 9]) and (want[0][:, 9] == 0).all()
    assert same_bits(want[0][0, 4], -0.0) and same_bits(want[0][1, 4], 0.0)         # the bits of a zero are its sign too
    assert want[0][0, 5] == -np.inf and want[0][1, 5] == np.inf
    if path == "packed" and N >= 600:
        # the three-valued feature keeps a third of the sample a candidate: forced to pack whatever fits, the call packs that too
        assert E.quantiles_last_path()[0]


def test_ties_that_keep_every_key_a_candidate_stay_on_the_ring(monkeypatch):
    """room for 500 candidates: a three-valued feature keeps 2100 and never packs, a continuous one packs after a digit or two; left
    to itself the library walks the ring"""
    for name in ("PTM_QUANTILES_PATH", "PTM_QUANTILES_PACK_BYTES", "PTM_QUANTILES_TILE"):
        monkeypatch.delenv(name, raising=False)
    x = adversarial_features(2100, 1)[:, 1:2].reshape(700, 3, 1)
    y = Q.skewed_series(700, 3, 1, 5)
    want_x, want_y = Q.quantiles(x, PROBS), Q.quantiles(y, PROBS)
    assert_same(E.quantiles_series(y, PROBS, brackets=True), want_y, "default")
    packed, ring_passes, packed_passes = E.quantiles_last_path()
    assert not packed and ring_passes >= 2 and packed_passes == 0
    monkeypatch.setenv("PTM_QUANTILES_PATH", "packed")
    monkeypatch.setenv("PTM_QUANTILES_PACK_BYTES", "4000")
    assert_same(E.quantiles_series(x, PROBS, brackets=True), want_x, "three values")
    assert E.quantiles_last_path() == (False, 8, 0)
    assert_same(E.quantiles_series(y, PROBS, brackets=True), want_y, "a continuous feature")
    packed, ring_passes, packed_passes = E.quantiles_last_path()
    assert packed and ring_passes >= 1 and packed_passes >= 1


def test_series_refusals():
    x = Q.skewed_series(6, 5, 3, 1)
    out = tuple(np.full((2, 3), -7.0) for _ in range(3))
    for nrows, probs in ((0, [0.5, 0.6]), (-1, [0.5, 0.6]), (7, [0.5, 0.6]), (3, [0.5, 1.5]), (3, [-0.1, 0.5]), (3, [np.nan, 0.5])):
        with pytest.raises(E.PtmError) as ei:
            E.quantiles_series(x, probs, nrows, brackets=True, out=out)
        assert str(ei.value).startswith("ptm error -1:")
    for nq in (0, 33):
        with pytest.raises(E.PtmError):
            E.quantiles_series(x, [0.5] * nq, 3, out=(np.full((max(nq, 1), 3), -7.0),))
    bad = x.copy()
    bad[5, 4, 2] = np.nan
    with pytest.raises(E.PtmError) as ei:
        E.quantiles_series(bad, [0.5, 0.6], 3, brackets=True, out=out)
    assert "NaN" in str(ei.value)
    assert all((o == -7.0).all() for o in out)


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


def ring_want(hist, nh, rung, nfeat, nrows, probs=PROBS, add=ADD, walkers=W):
    ok, win = R.ring_window(hist, slice(rung * walkers, (rung + 1) * walkers), add, nh[rung], nrows)
    assert ok
    return Q.quantiles(win[:, :, :nfeat], probs), win


@pytest.fixture(scope="module")
def ring():
    eng = run_engine(1 + STEPS // ADD + 99)
    hist = eng.history()
    nh = eng.nhist.reshape(NT, W)
    assert (nh[:HR] == STEPS).all()
    yield eng, hist, nh
    eng.close()


@pytest.mark.parametrize("rung,nfeat", [(0, 3), (1, 3), (0, 2), (1, 1)])
def test_engine_ring_equals_the_model_and_the_series_call(ring, rung, nfeat, path):
    eng, hist, nh = ring
    _, rows = ring_want(hist, nh, rung, DIM, STEPS // ADD)         # every saved row behind the start state
    for nrows in (1, 5, 1500):
        want, _ = ring_want(hist, nh, rung, nfeat, nrows)
        got = eng.posterior_quantiles(PROBS, rung, nfeat, nrows, brackets=True)
        assert_same(got, want, (rung, nfeat, nrows, path))
        check_path(path)
        assert_same(E.quantiles_series(rows[:, :, :nfeat], PROBS, nrows, brackets=True), got, ("series", rung, nfeat, nrows, path))
        assert np.isfinite(got[0]).all() and (got[0][0] <= got[0][1]).all() and (got[0][1] <= got[0][2]).all()
    if nfeat == DIM:                                                # the default: all features, every row every walker still has
        q, n = eng.posterior_quantiles(PROBS, rung)
        assert n == W * 1500 and same_bits(q, ring_want(hist, nh, rung, DIM, 1500)[0][0])


@pytest.mark.parametrize("nfeat", [20, 5])
def test_ring_in_the_permuted_layout_of_32_dimensions(nfeat, path):
    dim, steps = 20, 300
    eng = run_engine(steps + 20, dim=dim, nt=2, steps=steps, add=1, hr=1)
    try:
        hist, nh = eng.history(), eng.nhist.reshape(2, W)
        assert (nh[0] == steps).all()
        for nrows in (1, 150, 300):
            ok, win = R.ring_window(hist, slice(0, W), 1, nh[0], nrows)
            assert ok
            got = eng.posterior_quantiles(PROBS, 0, nfeat, nrows, brackets=True)
            assert_same(got, Q.quantiles(win[:, :, :nfeat], PROBS), (nfeat, nrows, path))
            assert len({v.tobytes() for v in got[0].T}) == nfeat    # the features are told apart
    finally:
        eng.close()


def test_walkers_with_different_add_state_counts_each_use_their_own_window(path):
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
                assert_same(eng.posterior_quantiles(PROBS, rung, nfeat, nrows, brackets=True), want, (rung, nfeat, nrows, path))
    finally:
        eng.close()


def test_wrapped_ring(path):
    cap = 1300
    eng = run_engine(cap)
    try:
        hist, nh = eng.history(), eng.nhist.reshape(NT, W)
        assert hist["row"].max() == STEPS // ADD and hist["row"][hist["row"] >= 0].min() > 1     # slots have wrapped
        for rung, nfeat, nrows in ((0, 3, 1000), (1, 2, 1300), (1, 3, 1)):                       # windows the ring still holds
            want, _ = ring_want(hist, nh, rung, nfeat, nrows)
            assert_same(eng.posterior_quantiles(PROBS, rung, nfeat, nrows, brackets=True), want, (rung, nfeat, nrows, path))
            check_path(path)
        assert same_bits(eng.posterior_quantiles(PROBS, 0)[0], ring_want(hist, nh, 0, DIM, cap)[0][0])
        # a window that reaches a row the ring has lost: refused, and the caller's arrays stay as they were
        assert not R.ring_window(hist, slice(0, W), ADD, nh[0], cap + 2)[0]
        out = tuple(np.full((3, DIM), -7.0) for _ in range(3))
        with pytest.raises(E.PtmError) as ei:
            eng.posterior_quantiles(PROBS, 0, DIM, cap + 2, brackets=True, out=out)
        assert "history_capacity must hold the window" in str(ei.value)
        assert all((o == -7.0).all() for o in out)
    finally:
        eng.close()


def test_ragged_counts_in_a_wrapped_ring(path):
    """walkers that differ in their counts, in a ring that has wrapped: every walker's own newest `capacity` rows are there and make
    the largest window; one row more is refused"""
    nt, steps, cap = 8, 3000, 1000
    eng = run_engine(cap, nt=nt, steps=steps, swap_rate=0.3, seed=0x5EED0E56)
    try:
        hist, nh = eng.history(), eng.nhist.reshape(nt, W)
        assert len(set(nh[1].tolist())) >= 3
        want, _ = ring_want(hist, nh, 1, DIM, cap)
        assert_same(eng.posterior_quantiles(PROBS, 1, DIM, cap, brackets=True), want, ("a full ring", path))
        out = tuple(np.full((3, DIM), -7.0) for _ in range(3))
        with pytest.raises(E.PtmError):
            eng.posterior_quantiles(PROBS, 1, DIM, cap + 1, brackets=True, out=out)
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
            got = aged.posterior_quantiles(PROBS, rung, nfeat, nrows, brackets=True)
            assert_same(got, Q.quantiles(win[:, :, :nfeat], PROBS), ("aged", rung, nfeat, nrows))
            assert_same(got, young.posterior_quantiles(PROBS, rung, nfeat, nrows, brackets=True), ("young twin", rung, nfeat, nrows))
        AU.age_engine(aged, young.step_count, (AU.COUNT_MAX - AU.MARGIN - int(aged.nhist.max())) // unit * unit, add)
        assert 2000000000 < aged.nhist.max()
        out = tuple(np.full((3, D), -7.0) for _ in range(3))
        with pytest.raises(E.PtmError) as err:
            aged.posterior_quantiles(PROBS, 1, D, 74, brackets=True, out=out)
        assert str(err.value).startswith("ptm error -2:") and "more than 2e9 steps" in str(err.value)
        assert all((o == -7.0).all() for o in out)
    finally:
        young.close(); aged.close()


def test_refusals(ring):
    eng, _, _ = ring
    assert np.isfinite(eng.posterior_quantiles(PROBS, 0, DIM, 500)[0]).all()
    out = tuple(np.full((3, DIM + 1), -7.0) for _ in range(3))
    for rung, nfeat, nrows in ((0, DIM, 0), (0, DIM, -2), (0, 0, 500), (0, DIM + 1, 500), (HR, DIM, 500), (0, DIM, STEPS // ADD + 1), (-1, DIM, 500)):
        with pytest.raises(E.PtmError) as ei:
            eng.posterior_quantiles(PROBS, rung, nfeat, nrows, brackets=True, out=out)
        assert str(ei.value).startswith("ptm error -1:")
    for probs in ([0.5, 0.5, 1.0000001], [0.5, -1e-9, 0.5], [0.5, 0.5, np.nan], [], [0.5] * 33):
        with pytest.raises(E.PtmError):
            eng.posterior_quantiles(probs, 0, DIM, 500, brackets=True, out=out)
    with pytest.raises(E.PtmError):
        eng.posterior_quantiles(PROBS, HR)                          # (also with the default window)
    with eng.batch():
        with pytest.raises(E.PtmError):
            eng.posterior_quantiles(PROBS, 0, DIM, 500, brackets=True, out=out)     # between batch_begin and batch_end
    assert all((o == -7.0).all() for o in out)
    plain = E.Engine(DIM, NT, 4)
    try:
        with pytest.raises(E.PtmError):
            plain.posterior_quantiles(PROBS, 0, DIM, 4)             # no history ring
    finally:
        plain.close()
    lone = run_engine(20, steps=10, walkers=1)                      # one walker, one row: a single sample is every quantile
    try:
        (want, _) = ring_want(lone.history(), lone.nhist.reshape(NT, 1), 0, DIM, 1, walkers=1)
        got = lone.posterior_quantiles(PROBS, 0, DIM, 1, brackets=True)
        assert_same(got, want, "one sample")
        assert got[3] == 1 and same_bits(got[0], got[1]) and same_bits(got[0], got[2])
    finally:
        lone.close()
    assert np.isfinite(eng.posterior_quantiles(PROBS, 0, DIM, 500)[0]).all()   # the engine is none the worse for it
