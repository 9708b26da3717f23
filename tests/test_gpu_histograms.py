"""Corner-plot histograms of a rung on the device (ptm_histograms, ptm_histograms_series): the kernels of
ptmcmc_amd/csrc/ptm_histograms_kernels.hpp count what the facade's histogram_estimator counts, so every count must equal the
Python twin's (tests/histograms_model.py, pinned to the facade and to numpy by tests/test_histograms_model_cpu.py) -- np.array_equal
on int64 -- whatever the pairs of an LDS tile and the mapping of the adds to the lanes that the environment forces."""
import numpy as np
import pytest

import histograms_model as H
import rhat_model as R
from ptmcmc_amd import engine as E
from ptmcmc_amd.problems import GaussianProblem

pytestmark = pytest.mark.gpu

NAMES = ("h1", "h2", "below", "above", "count")
TILES = {
    "default": {},
    "tile of one": {"PTM_HIST_TILE": "1"},
    "uneven tiles": {"PTM_HIST_TILE": "7"},
    "lanes over rows": {"PTM_HIST_MAP": "rows", "PTM_HIST_TILE": "5"},
}


@pytest.fixture(params=list(TILES))
def tile(request, monkeypatch):
    for name in ("PTM_HIST_TILE", "PTM_HIST_MAP"):
        monkeypatch.delenv(name, raising=False)
    for name, value in TILES[request.param].items():
        monkeypatch.setenv(name, value)
    return request.param


def assert_same(got, want, what):
    assert len(got) == len(want) == 5
    for name, g, w in zip(NAMES, got, want):
        if w is None:
            assert g is None, (what, name)
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == np.int64 or name == "count", (what, name, g.dtype)
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, np.argwhere(g != w)[:4] if g.shape == w.shape else (g.shape, w.shape))


def check_launch(tile, npairs, nbins):
    """the call that just ran used the tile and the mapping that were forced"""
    tiles, tp, mapping = E.histograms_last_launch()
    if npairs == 0:
        assert tiles == 0
        return
    assert tiles == -(-npairs // tp) and tp * nbins * nbins * 4 <= 128 * 1024 or tp == 1
    forced = int(TILES[tile].get("PTM_HIST_TILE", "0"))
    if forced:
        assert tp == min(forced, npairs, max(1, 128 * 1024 // (4 * nbins * nbins)))
    assert mapping == ("rows" if TILES[tile].get("PTM_HIST_MAP") == "rows" else "pairs")


def check_sums(x, lo, hi, nbins, got):
    """what the counts owe each other: every sample of a feature is below, above or in a bin; a pair's table holds the rows with both
    values inside, and its sum over the second feature's bins is the first feature's histogram of those rows"""
    h1, h2, below, above, count = got
    nf = h1.shape[0]
    assert count == x.shape[0] and np.array_equal(below + above + h1.sum(axis=1), np.full(nf, count) - np.isnan(x).sum(axis=0))
    if h2 is None:
        return
    k = np.stack([H.bins(x[:, f], lo[f], hi[f], nbins)[0] for f in range(nf)], axis=1)
    for i, j in H.pairs(nf):
        p = H.pair_index(nf, i, j)
        both = (k[:, i] >= 0) & (k[:, j] >= 0)
        assert h2[p].sum() == both.sum()
        assert np.array_equal(h2[p].sum(axis=1), np.bincount(k[both, i], minlength=nbins))
        assert np.array_equal(h2[p].sum(axis=0), np.bincount(k[both, j], minlength=nbins))


def series_case(series, nrows, lo, hi, nbins, what, tile, pairs=True):
    win = H.series_window(series, nrows)
    want = H.histograms(win, lo, hi, nbins, pairs)
    got = E.histograms_series(series, lo, hi, nbins, nrows, pairs=pairs)
    assert_same(got, want, (what, tile))
    nf = series.shape[2]
    check_launch(tile, nf * (nf - 1) // 2 if pairs else 0, nbins)
    check_sums(win.reshape(-1, nf), lo, hi, nbins, got)
    return got


def random_series(n, ns, nf, seed):
    """a different level and width per feature; the ranges cut a little off both tails"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, ns, nf)) * (1.0 + np.arange(nf) % 5) + 3.0 * np.arange(nf)
    lo, hi = 3.0 * np.arange(nf) - 1.7 * (1.0 + np.arange(nf) % 5), 3.0 * np.arange(nf) + 2.1 * (1.0 + np.arange(nf) % 5)
    return x, lo, hi


# ---- a caller's series ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [1, 3, 64, 65, 130])
def test_series_counts(ns, tile):
    """around the 64 walkers of a workgroup of the 2-D kernel, the 512 lanes of the 1-D kernel's, and the rows whose loads are asked
    early (8); 700 rows of 3 series cross a chunk of rows"""
    x, lo, hi = random_series(9, ns, 3, 10 + ns)
    for nrows in (1, 2, 7, 8, 9):
        got = series_case(x, nrows, lo, hi, 20, (ns, nrows), tile)
        assert got[4] == ns * nrows
    if ns == 3:
        x, lo, hi = random_series(700, 3, 3, 5)
        series_case(x, 700, lo, hi, 20, "rows in chunks", tile)
        series_case(x, 699, lo, hi, 20, "rows in chunks, not all", tile)


def test_chunks_of_several_rows(tile):
    """a launch is about 1024 workgroups (2048 of the 1-D kernel): 2500 rows of one series are chunks of two and of three rows, the
    last one short; 900 rows of 64 series of 130 features are chunks of eleven rows of the 1-D kernel, its loads asked 8 rows early"""
    x, lo, hi = random_series(2500, 1, 2, 77)
    series_case(x, 2500, lo, hi, 20, "one series", tile)
    x, lo, hi = random_series(900, 64, 130, 78)
    series_case(x, 900, lo, hi, 5, "130 features", tile, pairs=False)


@pytest.mark.parametrize("nf,nbins", [(1, 20), (2, 20), (3, 1), (3, 2), (3, 127), (33, 20), (5, 128), (70, 3)])
def test_feature_and_bin_counts(nf, nbins, tile):
    """no pair, one pair, 528 pairs in seven tiles of 81; 128 bins: two pairs a tile, ten pairs in five; 70 features: two tiles of the
    1-D kernel"""
    x, lo, hi = random_series(5, 65, nf, nf + nbins)
    got = series_case(x, 5, lo, hi, nbins, (nf, nbins), tile)
    if nf == 1:
        assert got[1].shape == (0, nbins, nbins)
    if tile == "default" and (nf, nbins) in (((33, 20)), ((5, 128))):
        assert E.histograms_last_launch()[:2] == ((7, 81) if nf == 33 else (5, 2))
    series_case(x, 4, lo, hi, nbins, (nf, nbins, "no pairs"), tile, pairs=False)


def test_the_cap_of_the_pair_counters(monkeypatch):
    """npairs * nbins^2 <= 2^25.  n (n - 1) / 2 is a power of two for n = 2 alone, so no shape meets the cap exactly: 64 features at
    128 bins are the largest below it (2016 * 16384 = 2^25 - 2^19 counters), one feature more (2080 pairs) is refused; at one bin
    8192 features (2^25 - 4096 pairs) pass and 8193 do not"""
    for name in ("PTM_HIST_TILE", "PTM_HIST_MAP"):
        monkeypatch.delenv(name, raising=False)
    rng = np.random.default_rng(3)
    x = rng.uniform(0, 1, (2, 3, 65))
    lo, hi = np.zeros(65), np.ones(65)
    h1, h2, below, above, n = E.histograms_series(x[:, :, :64], lo[:64], hi[:64], 128)
    assert n == 6 and h2.shape == (2016, 128, 128) and (h2.reshape(2016, -1).sum(axis=1) == 6).all()
    k = np.floor(x.reshape(6, 65) * 128).astype(int)                # (multiples of 1/128 are exact: the bins of [0, 1) by 128)
    assert np.array_equal(h1, np.stack([np.bincount(k[:, f], minlength=128) for f in range(64)]))
    for i, j in ((0, 1), (0, 63), (31, 40), (62, 63)):
        want = np.zeros((128, 128), dtype=np.int64)
        np.add.at(want, (k[:, i], k[:, j]), 1)
        assert np.array_equal(h2[H.pair_index(64, i, j)], want)
    assert E.histograms_last_launch()[:2] == (1008, 2)
    out = (np.full((65, 128), -7, dtype=np.int64), np.full((1, 128, 128), -7, dtype=np.int64), np.full(65, -7, dtype=np.int64), np.full(65, -7, dtype=np.int64))
    with pytest.raises(E.PtmError) as ei:
        E.histograms_series(x, lo, hi, 128, out=out)
    assert str(ei.value).startswith("ptm error -2:") and all((o == -7).all() for o in out)
    assert E.histograms_series(x, lo, hi, 128, pairs=False)[0].sum() == 6 * 65      # (without the pairs there is no cap)
    wide = rng.uniform(0, 1, (1, 1, 8193))
    h1, h2, _, _, _ = E.histograms_series(wide[:, :, :8192], np.zeros(8192), np.ones(8192), 1)
    assert h2.shape == (8192 * 8191 // 2, 1, 1) and (h2 == 1).all() and (h1 == 1).all()
    with pytest.raises(E.PtmError) as ei:
        E.histograms_series(wide, np.zeros(8193), np.ones(8193), 1)
    assert str(ei.value).startswith("ptm error -2:")


def adversarial_case(nbins, ns):
    lo_u, hi_u = H.ulps_wide_range()
    ranges = [(-3.0, 5.0), (0.0, 1.0), (lo_u, hi_u), (-1e5, 1e5), (2.5e-6, 2.5e-6 + 1e-9), (1e-5, 3e-5), (0.0, 7.0), (10.0, 11.0), (-11.0, -10.0)]
    x = H.adversarial_series(ranges[:6], nbins, ns, seed=nbins)
    n = x.shape[0]
    rng = np.random.default_rng(nbins + ns)
    extra = np.empty((n, ns, 4))
    extra[..., 0] = 7.0                                             # every value equal to hi: the closed last bin
    extra[..., 1] = rng.uniform(0.0, 9.0, (n, ns))                  # wholly below its range
    extra[..., 2] = rng.uniform(0.0, 9.0, (n, ns))                  # wholly above
    extra[..., 3] = np.where(rng.integers(0, 2, (n, ns)) == 1, 0.0, -0.0)   # zeros of both signs with lo = 0
    x = np.concatenate([x, extra], axis=2)
    lo = np.array([r[0] for r in ranges] + [0.0])
    hi = np.array([r[1] for r in ranges] + [1.0])
    return x, lo, hi


@pytest.mark.parametrize("nbins", [1, 2, 20, 127, 128])
def test_adversarial_values(nbins, tile):
    """every edge and its two neighbours in the doubles, lo, hi, +-0, +-inf and far values, in ranges of different size -- one 300
    ulps wide at 1.0, where the guess of a bin is worthless"""
    x, lo, hi = adversarial_case(nbins, 3)
    for f in range(lo.size):
        assert H.edges_ok(lo[f], hi[f], nbins), f
    n = x.shape[0]
    h1, h2, below, above, count = series_case(x, n, lo, hi, nbins, nbins, tile)
    assert h1[6, nbins - 1] == count and below[6] == above[6] == 0              # x == hi everywhere
    assert below[7] == count and above[8] == count and h1[7].sum() == h1[8].sum() == 0
    assert h1[9, 0] == count                                                    # -0.0 compares as 0: bin 0 of [0, 1]
    assert (h2[H.pair_index(10, 6, 9)] == np.where(np.arange(nbins * nbins).reshape(nbins, nbins) == (nbins - 1) * nbins, count, 0)).all()
    assert h2[H.pair_index(10, 0, 7)].sum() == 0                                # a feature outside its range empties its pairs only
    assert np.isinf(x[..., 0]).sum() >= 2 and below[0] >= 1 and above[0] >= 1


def test_series_refusals():
    x, lo, hi = random_series(6, 5, 3, 1)
    mk = lambda: (np.full((3, 4), -7, dtype=np.int64), np.full((3, 4, 4), -7, dtype=np.int64), np.full(3, -7, dtype=np.int64), np.full(3, -7, dtype=np.int64))
    out = mk()
    bad_lo = lambda i, v: np.concatenate([lo[:i], [v], lo[i + 1:]])
    lo_u, hi_u = H.ulps_wide_range(3)
    cases = [(0, 4, lo, hi), (-1, 4, lo, hi), (7, 4, lo, hi), (3, 0, lo, hi), (3, 129, lo, hi), (3, -1, lo, hi),
             (3, 4, bad_lo(1, np.nan), hi), (3, 4, bad_lo(1, -np.inf), hi), (3, 4, bad_lo(2, hi[2]), hi), (3, 4, bad_lo(0, hi[0] + 1), hi), (3, 4, lo, bad_lo(0, np.inf)),
             (3, 4, bad_lo(0, lo_u), np.concatenate([[hi_u], hi[1:]])),        # three ulps cannot hold four bins
             (3, 4, bad_lo(0, -1e308), np.concatenate([[1e308], hi[1:]]))]     # hi - lo overflows
    for nrows, nbins, a, b in cases:
        with pytest.raises(E.PtmError) as ei:
            E.histograms_series(x, a, b, nbins, nrows, out=out if nbins == 4 else mk())
        assert str(ei.value).startswith("ptm error -1:"), (nrows, nbins)
    assert not H.edges_ok(lo_u, hi_u, 4)
    with pytest.raises(E.PtmError) as ei:
        E.histograms_series(x, bad_lo(0, lo_u), np.concatenate([[hi_u], hi[1:]]), 4, 3, out=out)
    assert "the range cannot hold nbins bins" in str(ei.value)
    bad = x.copy()
    bad[5, 4, 2] = np.nan
    with pytest.raises(E.PtmError) as ei:
        E.histograms_series(bad, lo, hi, 4, 3, out=out)
    assert "NaN" in str(ei.value)
    assert all((o == -7).all() for o in out)
    with pytest.raises(ValueError):
        E.histograms_series(x, lo[:2], hi, 4)
    assert_same(E.histograms_series(x, lo, hi, 4, 3, out=out), H.histograms(x[3:], lo, hi, 4), "the same arrays, filled")


# ---- the engine's history ring --------------------------------------------------------------------------------------------------
DIM, NT, W, ADD, HR, STEPS = 3, 4, 70, 2, 2, 3000
NBINS = 20


def run_engine(capacity, dim=DIM, nt=NT, steps=STEPS, add=ADD, hr=HR, swap_rate=0.1, seed=0x5EED0E57, walkers=W):
    pr = GaussianProblem(dim, nt, 1e2)
    eng = E.Engine(dim, nt, walkers, seed=seed, swap_rate=swap_rate, add_every_n=add, history_rungs=hr, history_capacity=capacity)
    pr.configure(eng, E.PROP_LOWER)
    eng.init_from_prior()
    eng.step(steps)
    eng.sync()
    return eng


def ranges_of(win, nfeat, shrink):
    """shrink = 0: the sample's own minimum and maximum (corner's default); else cut that share of the width off both ends"""
    flat = win[:, :, :nfeat].reshape(-1, nfeat)
    a, b = flat.min(axis=0), flat.max(axis=0)
    return a + shrink * (b - a), b - shrink * (b - a)


def ring_case(eng, hist, nh, rung, nfeat, nrows, what, add=ADD, walkers=W, nbins=NBINS):
    ok, win = R.ring_window(hist, slice(rung * walkers, (rung + 1) * walkers), add, nh[rung], nrows)
    assert ok
    got = None
    for shrink in (0.0, 0.2):
        lo, hi = ranges_of(win, nfeat, shrink)
        if not all(H.edges_ok(lo[f], hi[f], nbins) for f in range(nfeat)):
            lo, hi = lo - 0.5, hi + 0.5                             # (a window of one row: numpy's widening of an empty range)
        want = H.histograms(win[:, :, :nfeat], lo, hi, nbins)
        got = eng.posterior_histograms(lo, hi, nbins, rung, nfeat, nrows)
        assert_same(got, want, (what, rung, nfeat, nrows, shrink))
        check_sums(win[:, :, :nfeat].reshape(-1, nfeat), lo, hi, nbins, got)
        if shrink == 0.0 and nrows > 1:
            assert (got[2] == 0).all() and (got[3] == 0).all() and (got[0].sum(axis=1) == walkers * nrows).all()
    return got, win


@pytest.fixture(scope="module")
def ring():
    eng = run_engine(1 + STEPS // ADD + 99)
    hist = eng.history()
    nh = eng.nhist.reshape(NT, W)
    assert (nh[:HR] == STEPS).all()
    yield eng, hist, nh
    eng.close()


@pytest.mark.parametrize("rung,nfeat", [(0, 3), (1, 3), (0, 2), (1, 1)])
def test_engine_ring_equals_the_model_and_the_series_call(ring, rung, nfeat, tile):
    eng, hist, nh = ring
    ok, rows = R.ring_window(hist, slice(rung * W, (rung + 1) * W), ADD, nh[rung], STEPS // ADD)     # every saved row behind the start state
    assert ok
    for nrows in (1, 5, 1500):
        got, win = ring_case(eng, hist, nh, rung, nfeat, nrows, tile)
        lo, hi = ranges_of(win, nfeat, 0.2)
        if nrows > 1:
            assert_same(E.histograms_series(rows[:, :, :nfeat], lo, hi, NBINS, nrows), got, ("series", rung, nfeat, nrows, tile))
            check_launch(tile, nfeat * (nfeat - 1) // 2, NBINS)
    if nfeat == DIM:                                                # the defaults: all features, every row every walker still has, 20 bins
        _, win = ring_case(eng, hist, nh, rung, DIM, 1500, "for the default")
        lo, hi = ranges_of(win, DIM, 0.0)
        assert_same(eng.posterior_histograms(lo, hi, rung=rung), H.histograms(win, lo, hi, 20), "defaults")
        h1, h2, below, above, n = eng.posterior_histograms(lo, hi, rung=rung, pairs=False)
        assert h2 is None and n == W * 1500 and np.array_equal(h1, np.stack([np.histogram(win[..., f].ravel(), 20, (lo[f], hi[f]))[0] for f in range(DIM)]))


@pytest.mark.parametrize("nfeat", [20, 5])
def test_ring_in_the_permuted_layout_of_32_dimensions(nfeat, tile):
    """the rows of the 32-dimension kernels lie permuted in the ring (ess_pos)"""
    dim, steps = 20, 120
    eng = run_engine(steps + 20, dim=dim, nt=2, steps=steps, add=1, hr=1)
    try:
        hist, nh = eng.history(), eng.nhist.reshape(2, W)
        assert (nh[0] == steps).all()
        for nrows in (1, steps // 2, steps):
            got, _ = ring_case(eng, hist, nh, 0, nfeat, nrows, (dim, tile), add=1, nbins=10)
        assert len({v.tobytes() for v in got[0]}) == nfeat          # the features are told apart
    finally:
        eng.close()


@pytest.mark.parametrize("name,nfeat", [("C", 40), ("C", 9), ("D", 100), ("D", 11)])
def test_rings_of_the_64_and_128_dimension_kernels(name, nfeat, tile):
    """the rings of tests/history_readers_util.py that the 64- and 128-dimension sweep kernels record: three walkers, permuted rows"""
    import history_readers_util as HU
    ring = HU.RINGS[name]
    assert ring.permuted and ring.W == 3
    eng = HU.ring_engine(ring)
    try:
        eng.step(60)
        eng.sync()
        hist, nh = eng.history(), eng.nhist.reshape(ring.Nt, ring.W)
        for rung, nrows in ((0, 30), (1, 7)):
            ring_case(eng, hist, nh, rung, nfeat, nrows, (name, tile), add=ring.add, walkers=ring.W, nbins=6)
    finally:
        eng.close()


def test_walkers_with_different_add_state_counts_each_use_their_own_window(tile):
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
                ring_case(eng, hist, nh, rung, nfeat, nrows, tile)
    finally:
        eng.close()


def test_wrapped_ring(tile):
    cap = 1300
    eng = run_engine(cap)
    try:
        hist, nh = eng.history(), eng.nhist.reshape(NT, W)
        assert hist["row"].max() == STEPS // ADD and hist["row"][hist["row"] >= 0].min() > 1     # slots have wrapped
        for rung, nfeat, nrows in ((0, 3, 1000), (1, 2, 1300), (1, 3, 1)):                       # windows the ring still holds
            ring_case(eng, hist, nh, rung, nfeat, nrows, tile)
        _, win = ring_case(eng, hist, nh, 0, DIM, cap, "a full ring")
        lo, hi = ranges_of(win, DIM, 0.0)
        assert_same(eng.posterior_histograms(lo, hi), H.histograms(win, lo, hi, 20), "the default window of a wrapped ring")
        # a window that reaches a row the ring has lost: refused, and the caller's arrays stay as they were
        assert not R.ring_window(hist, slice(0, W), ADD, nh[0], cap + 2)[0]
        out = (np.full((DIM, 20), -7, dtype=np.int64), np.full((3, 20, 20), -7, dtype=np.int64), np.full(DIM, -7, dtype=np.int64), np.full(DIM, -7, dtype=np.int64))
        with pytest.raises(E.PtmError) as ei:
            eng.posterior_histograms(lo, hi, 20, 0, DIM, cap + 2, out=out)
        assert "history_capacity must hold the window" in str(ei.value)
        assert all((o == -7).all() for o in out)
    finally:
        eng.close()


def test_ragged_counts_in_a_wrapped_ring(tile):
    """walkers that differ in their counts, in a ring that has wrapped: every walker's own newest `capacity` rows are there and make
    the largest window; one row more is refused"""
    nt, steps, cap = 8, 3000, 1000
    eng = run_engine(cap, nt=nt, steps=steps, swap_rate=0.3, seed=0x5EED0E56)
    try:
        hist, nh = eng.history(), eng.nhist.reshape(nt, W)
        assert len(set(nh[1].tolist())) >= 3
        _, win = ring_case(eng, hist, nh, 1, DIM, cap, tile)
        lo, hi = ranges_of(win, DIM, 0.0)
        out = (np.full((DIM, 20), -7, dtype=np.int64), np.full((3, 20, 20), -7, dtype=np.int64), np.full(DIM, -7, dtype=np.int64), np.full(DIM, -7, dtype=np.int64))
        with pytest.raises(E.PtmError):
            eng.posterior_histograms(lo, hi, 20, 1, DIM, cap + 1, out=out)
        assert all((o == -7).all() for o in out)
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
        lo, hi = np.full(D, -1.5), np.full(D, 2.0)
        for rung, nfeat, nrows in ((0, 2, 74), (1, 2, 74), (3, 1, 1)):
            ok, win = R.ring_window(hist, slice(rung * W, (rung + 1) * W), add, nh[rung], nrows)
            assert ok
            got = aged.posterior_histograms(lo[:nfeat], hi[:nfeat], 20, rung, nfeat, nrows)
            assert_same(got, H.histograms(win[:, :, :nfeat], lo, hi, 20), ("aged", rung, nfeat, nrows))
            assert_same(got, young.posterior_histograms(lo[:nfeat], hi[:nfeat], 20, rung, nfeat, nrows), ("young twin", rung, nfeat, nrows))
        AU.age_engine(aged, young.step_count, (AU.COUNT_MAX - AU.MARGIN - int(aged.nhist.max())) // unit * unit, add)
        assert 2000000000 < aged.nhist.max()
        out = (np.full((D, 20), -7, dtype=np.int64), np.full((1, 20, 20), -7, dtype=np.int64), np.full(D, -7, dtype=np.int64), np.full(D, -7, dtype=np.int64))
        with pytest.raises(E.PtmError) as err:
            aged.posterior_histograms(lo, hi, 20, 1, D, 74, out=out)
        assert str(err.value).startswith("ptm error -2:") and "more than 2e9 steps" in str(err.value)
        assert all((o == -7).all() for o in out)
    finally:
        young.close(); aged.close()


def test_refusals(ring):
    eng, _, _ = ring
    lo, hi = np.full(DIM + 1, -2.0), np.full(DIM + 1, 2.0)
    assert eng.posterior_histograms(lo[:DIM], hi[:DIM], 20, 0, DIM, 500)[0].sum() > 0
    mk = lambda nf: (np.full((nf, 20), -7, dtype=np.int64), np.full((max(nf * (nf - 1) // 2, 1), 20, 20), -7, dtype=np.int64), np.full(nf, -7, dtype=np.int64), np.full(nf, -7, dtype=np.int64))
    outs = []
    for rung, nfeat, nrows in ((0, DIM, 0), (0, DIM, -2), (0, 0, 500), (0, DIM + 1, 500), (HR, DIM, 500), (0, DIM, STEPS // ADD + 1), (-1, DIM, 500)):
        outs.append(mk(max(nfeat, 1)))
        with pytest.raises(E.PtmError) as ei:
            eng.posterior_histograms(lo[:nfeat], hi[:nfeat], 20, rung, nfeat, nrows, out=outs[-1])
        assert str(ei.value).startswith("ptm error -1:")
    out = mk(DIM)
    lo_u, hi_u = H.ulps_wide_range(3)
    for a, b, nbins in ((lo[:DIM], hi[:DIM], 0), (lo[:DIM], hi[:DIM], 129), (hi[:DIM], lo[:DIM], 20), (lo[:DIM], lo[:DIM], 20), (np.array([-2.0, np.nan, -2.0]), hi[:DIM], 20),
                        (lo[:DIM], np.array([2.0, 2.0, np.inf]), 20), (np.array([-2.0, lo_u, -2.0]), np.array([2.0, hi_u, 2.0]), 20)):
        with pytest.raises(E.PtmError) as ei:
            eng.posterior_histograms(a, b, nbins, 0, DIM, 500, out=out)
        assert str(ei.value).startswith("ptm error -1:")
    with pytest.raises(E.PtmError):
        eng.posterior_histograms(lo[:DIM], hi[:DIM], rung=HR)       # (also with the default window)
    with eng.batch():
        with pytest.raises(E.PtmError):
            eng.posterior_histograms(lo[:DIM], hi[:DIM], 20, 0, DIM, 500, out=out)     # between batch_begin and batch_end
    assert all((o == -7).all() for o in out) and all((o == -7).all() for t in outs for o in t)
    plain = E.Engine(DIM, NT, 4)
    try:
        with pytest.raises(E.PtmError):
            plain.posterior_histograms(lo[:DIM], hi[:DIM], 20, 0, DIM, 4)             # no history ring
    finally:
        plain.close()
    assert eng.posterior_histograms(lo[:DIM], hi[:DIM], 20, 0, DIM, 500)[0].sum() > 0   # the engine is none the worse for it
