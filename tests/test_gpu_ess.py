"""Effective sample size on the device (ptm_ess_*): the kernels of ptmcmc_amd/csrc/ptm_ess_kernels.hpp restate the facade's
ess_estimator with one lane per (series, feature), every sum in the host's order -- so their answers must carry the host
estimator's very bits (tests/ess_model.py is its line-by-line Python twin, pinned to the facade and to the real reference by
tests/test_ess_model_cpu.py)."""
import os
import tempfile

import numpy as np
import pytest

import ess_model as M
import golden_io
from ptmcmc_amd import engine as E
from ptmcmc_amd.problems import GaussianProblem

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def test_golden_series_match_the_reference_and_the_facade_bit_for_bit():
    g = golden_io.load("ess.json.gz")
    nonzero = searched = 0
    with tempfile.TemporaryDirectory() as d:
        exe = M.build_fixture_driver(d)
        for c in g["cases"]:
            series = M.golden_series(c)
            host = M.fixture_driver_answers(exe, series, c["queries"])
            for q, (h_ess, h_len) in zip(c["queries"], host):
                ess, length = E.effective_samples_series(series[:, None, :], q["width"], q["every"], q["esslimit"])
                print(q, float(ess[0]), int(length[0]), h_ess, h_len)
                assert int(length[0]) == q["length"], (q, ess, length)
                assert abs(ess[0] - q["ess"]) <= 1e-10 * max(1.0, abs(q["ess"])), (q, ess)
                assert int(length[0]) == h_len and same_bits(ess[0], h_ess), (q, float(ess[0]), h_ess)
                nonzero += q["ess"] > 0
                searched += q["esslimit"] >= 0 and q["ess"] > 0
    assert nonzero >= 15 and searched >= 5
    assert any(q["ess"] == 0 and q["length"] == 0 for c in g["cases"] for q in c["queries"])     # the too-short cases were there


# ---- many series, ragged shapes -------------------------------------------------------------------------------------------
N_AR, NS_AR, NF_AR, SEED_AR = 6000, 70, 3, 1
AR_SHAPES = [(500, 1, 2), (500, 7, 2), (640, 3, 4)]


def ar1_series():
    rng = np.random.default_rng(SEED_AR)
    phi = rng.uniform(0.2, 0.97, size=(NS_AR, NF_AR))
    e = rng.standard_normal((N_AR, NS_AR, NF_AR))
    x = np.empty_like(e)
    cur = np.zeros((NS_AR, NF_AR))
    for t in range(N_AR):
        cur = phi * cur + e[t]
        x[t] = cur
    return x


@pytest.fixture(scope="module")
def ar1():
    x = ar1_series()
    est = M.Estimator(N_AR, NS_AR, NF_AR, M.series_reader(x))
    return x, {s: est.windowed(*s, detail=True) for s in AR_SHAPES}


@pytest.mark.parametrize("shape", AR_SHAPES)
def test_many_series_of_ragged_shape_equal_the_model(ar1, shape):
    x, want = ar1
    w_ess, w_nwin, w_feat = want[shape]
    # the case can tell series and features apart: several winning n, and not one feature setting every minimum
    assert len(set(w_nwin.tolist())) >= 3 and len(set(w_feat.tolist())) >= 2, (sorted(set(w_nwin.tolist())), sorted(set(w_feat.tolist())))
    if shape[0] % shape[1]:
        assert (shape[0] // shape[1]) * shape[1] < shape[0]          # span < width
    ess, nwin = E.ess_series_windowed(x, *shape)
    bad = [s for s in range(NS_AR) if not same_bits(ess[s], w_ess[s]) or nwin[s] != w_nwin[s]]
    assert not bad, (shape, bad[:5], ess[bad[:5]], w_ess[bad[:5]], nwin[bad[:5]], w_nwin[bad[:5]])


# ---- the engine's history ring ------------------------------------------------------------------------------------------------
DIM, NT, W, ADD, HR, STEPS = 3, 4, 70, 2, 2, 3000
RING_SHAPES = [(200, 2, 2), (210, 3, 2), (150, 1, 3)]      # stride a multiple of add_every_n (rows linear in the sample number), and not


def run_engine(capacity):
    pr = GaussianProblem(DIM, NT, 1e2)
    eng = E.Engine(DIM, NT, W, seed=0x5EED0E55, swap_rate=0.1, add_every_n=ADD, history_rungs=HR, history_capacity=capacity)
    pr.configure(eng, E.PROP_LOWER)
    eng.init_from_prior()
    eng.step(STEPS)
    eng.sync()
    return eng


@pytest.fixture(scope="module")
def ring():
    eng = run_engine(1 + STEPS // ADD + 99)
    hist = eng.history()
    nh = eng.nhist.reshape(NT, W)
    assert (nh[:HR] == STEPS).all()
    yield eng, hist
    eng.close()


def ring_model(hist, rung, nfeat):
    return M.Estimator(STEPS, W, nfeat, M.ring_reader(hist, slice(rung * W, (rung + 1) * W), ADD))


@pytest.mark.parametrize("rung,nfeat", [(0, 3), (1, 3), (0, 2)])
def test_engine_ring_equals_the_model_and_the_series_calls(ring, rung, nfeat):
    eng, hist = ring
    est = ring_model(hist, rung, nfeat)
    series = M.ring_series(hist, slice(rung * W, (rung + 1) * W), ADD, STEPS)[:, :, :nfeat]
    for shape in RING_SHAPES:
        w_ess, w_nwin = est.windowed(*shape)
        assert (w_nwin > 0).all()
        ess, nwin = eng.ess_windowed(rung, nfeat, *shape)
        assert eng.ess_last_on_device
        assert same_bits(ess, w_ess) and np.array_equal(nwin, w_nwin), (shape, ess[:4], w_ess[:4], nwin[:4], w_nwin[:4])
        s_ess, s_nwin = E.ess_series_windowed(series, *shape)
        assert same_bits(ess, s_ess) and np.array_equal(nwin, s_nwin), shape
    for width, every, limit in ((100, 2, -1), (100, 1, 0.4)):
        w_ess, w_len = est.report(width, every, limit)
        ess, length = eng.effective_samples(rung, nfeat, width, every, limit)
        assert same_bits(ess, w_ess) and np.array_equal(length, w_len), (width, every, limit, ess[:4], w_ess[:4], length[:4], w_len[:4])
        s_ess, s_len = E.effective_samples_series(series, width, every, limit)
        assert same_bits(ess, s_ess) and np.array_equal(length, s_len)
    assert (eng.effective_samples(rung, nfeat, 100, 2)[0] > 0).all()


def test_wrapped_ring_skips_the_rows_it_has_lost():
    """a ring shorter than the run: the oldest lagged partners of the first window are gone, the device skips them as cold_row does"""
    eng = run_engine(1300)
    try:
        hist = eng.history()
        assert hist["row"].max() == STEPS // ADD and hist["row"][hist["row"] >= 0].min() > 1     # slots have wrapped
        shape = (400, 2, 2)
        for rung in (0, 1):
            est = ring_model(hist, rung, DIM)
            nwin, lags, _, _, count = est.table(*shape)
            assert count.min() >= 1 and count[0].min() < shape[0] // shape[1] and count[-1].min() == shape[0] // shape[1]
            w_ess, w_nwin = est.windowed(*shape)
            ess, n = eng.ess_windowed(rung, DIM, *shape)
            assert same_bits(ess, w_ess) and np.array_equal(n, w_nwin), (rung, ess[:4], w_ess[:4], n[:4], w_nwin[:4])
    finally:
        eng.close()


def test_walkers_with_different_add_state_counts_each_get_their_own_windows():
    """five exchange candidates per step: a rung exchanged twice in a step makes an extra add_state call, so the walkers of a rung
    differ in their step counts -- and with them in the number of windows and where these begin.  Every walker's answer is the
    model's for its own count; the report groups the walkers whose counts lead to the same passes."""
    nt, steps = 8, 3000
    pr = GaussianProblem(DIM, nt, 1e2)
    eng = E.Engine(DIM, nt, W, seed=0x5EED0E56, swap_rate=0.3, add_every_n=ADD, history_rungs=HR, history_capacity=1 + steps // ADD + 1500)
    try:
        pr.configure(eng, E.PROP_LOWER)
        eng.init_from_prior()
        eng.step(steps)
        eng.sync()
        assert eng.max_swaps == 5
        hist, nh = eng.history(), eng.nhist.reshape(nt, W)
        for rung in (0, 1):
            counts = nh[rung]
            print("rung", rung, "add_state counts", sorted(set(counts.tolist())))
            # (the coldest rung has one neighbour only and is never exchanged twice: its walkers agree; the rungs above do not)
            assert counts.min() >= steps and (len(set(counts.tolist())) >= 5 if rung else set(counts.tolist()) == {steps}), sorted(set(counts.tolist()))
            got = {"w1": eng.ess_windowed(rung, DIM, 200, 2, 2), "w2": eng.ess_windowed(rung, 2, 215, 3, 2),
                   "r2": eng.effective_samples(rung, DIM, 100, 1, 0.4), "r1": eng.effective_samples(rung, DIM, 100, 2)}
            assert eng.ess_last_on_device
            for c in sorted(set(counts.tolist())):
                who = np.flatnonzero(counts == c)
                rd = M.ring_reader(hist, rung * W + who, ADD)
                est3, est2 = M.Estimator(c, len(who), DIM, rd), M.Estimator(c, len(who), 2, rd)
                want = {"w1": est3.windowed(200, 2, 2), "w2": est2.windowed(215, 3, 2), "r1": est3.report(100, 2, -1), "r2": est3.report(100, 1, 0.4)}
                for k in want:
                    assert same_bits(got[k][0][who], want[k][0]) and np.array_equal(got[k][1][who], want[k][1]), (rung, c, k, got[k][0][who][:3], want[k][0][:3], got[k][1][who][:3], want[k][1][:3])
            assert (got["w1"][0] > 0).all() and (got["r1"][0] > 0).all()
    finally:
        eng.close()


def test_chunked_workspace_gives_the_same_bits(ring):
    eng, hist = ring
    shape = RING_SHAPES[0]
    whole = eng.ess_windowed(0, DIM, *shape)
    nwin, lags = STEPS // shape[0] - shape[2], M.lag_list(shape[1], shape[2], shape[0] // shape[1])
    per_series = DIM * nwin * (len(lags) * 20 + 8)           # bytes of one series' table
    chunk = 30
    assert -(-W // chunk) >= 3 and W % chunk
    old = os.environ.get("PTM_ESS_WORKSPACE_MB")
    os.environ["PTM_ESS_WORKSPACE_MB"] = repr((chunk + 0.5) * per_series / 2.0 ** 20)
    try:
        parts = eng.ess_windowed(0, DIM, *shape)
        rep = eng.effective_samples(0, DIM, 100, 2)
    finally:
        if old is None:
            del os.environ["PTM_ESS_WORKSPACE_MB"]
        else:
            os.environ["PTM_ESS_WORKSPACE_MB"] = old
    assert same_bits(parts[0], whole[0]) and np.array_equal(parts[1], whole[1])
    again = eng.effective_samples(0, DIM, 100, 2)
    assert same_bits(rep[0], again[0]) and np.array_equal(rep[1], again[1])


def test_refusals(ring):
    eng, _ = ring
    ess, _ = eng.ess_windowed(0, DIM, 200, 2, 2)
    assert eng.ess_last_on_device and (ess > 0).all()
    with pytest.raises(E.PtmError):
        eng.ess_windowed(HR, DIM, 200, 2, 2)                 # rung >= history_rungs
    assert not eng.ess_last_on_device
    with pytest.raises(E.PtmError):
        eng.effective_samples(0, DIM + 1, 100, 2)            # nfeat > dim
    with pytest.raises(E.PtmError):
        eng.ess_windowed(0, 0, 200, 2, 2)
    plain = E.Engine(DIM, NT, 4)
    try:
        with pytest.raises(E.PtmError):
            plain.effective_samples(0)                       # no history ring
    finally:
        plain.close()
    ess, nwin = eng.ess_windowed(0, DIM, 2000, 2, 2)         # too short for one window: (0, 0), and no kernel ran
    assert not ess.any() and not nwin.any() and not eng.ess_last_on_device
    eng.effective_samples(0, DIM, 100, 2)
    assert eng.ess_last_on_device
