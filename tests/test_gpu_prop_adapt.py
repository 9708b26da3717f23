"""Every rung's Gaussian proposal from its own sampled covariance, on the device: ptm_moments_rungs against ptm_moments rung by rung,
ptm_eigen_factors (ptmcmc_amd/csrc/ptm_eigen_kernels.hpp) against the twin of the facade's eigen_factor (tests/prop_adapt_model.py: its
recorded answers, which tests/test_prop_adapt_model_cpu.py holds the twin and the facade to), ptm_adapt_proposals against
ptm_set_proposal_rung on a second engine at every install target (tests/prop_adapt_cases.py), its status values and refusals, and a
statistics case in the form of tests/test_gpu_statistics.py."""
import numpy as np
import pytest

import prop_adapt_cases as PC
import prop_adapt_model as P
from ptmcmc_amd import engine as E
from ptmcmc_amd.problems import GaussianProblem

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


# ---- ptm_moments_rungs ------------------------------------------------------------------------------------------------------------
def run_engine(dim, nt, walkers, steps, add, cap, hr, swap_rate=0.1, seed=0x5EED0E57):
    eng = E.Engine(dim, nt, walkers, seed=seed, swap_rate=swap_rate, add_every_n=add, history_rungs=hr, history_capacity=cap)
    GaussianProblem(dim, nt, 1e2).configure(eng, E.PROP_LOWER)
    eng.init_from_prior()
    eng.step(steps)
    eng.sync()
    return eng


def assert_rungs_equal_single(eng, first, n, nfeat, nrows, cov=None):
    mean, c, var, count = eng.moments_rungs(first, n, nfeat, nrows, cov=cov)
    for r in range(n):
        m1, c1, v1, n1 = eng.posterior_moments(first + r, nfeat, nrows, cov=cov)
        assert same_bits(mean[r], m1) and same_bits(var[r], v1) and count == n1, (first + r, nfeat, nrows)
        assert (c is None and c1 is None) or same_bits(c[r], c1), (first + r, nfeat, nrows, "cov")
    return mean, c, var


def test_moments_rungs_equal_moments_rung_by_rung():
    """4 rungs x 70 walkers (two blocks of walkers, the second ragged) x 6 dimensions"""
    eng = run_engine(6, 4, 70, 40, 1, 64, 4)
    try:
        for nrows in (1, 5, 40):
            for nfeat in (1, 6):
                assert_rungs_equal_single(eng, 0, 4, nfeat, nrows)
        assert_rungs_equal_single(eng, 1, 2, 6, 5)
        assert_rungs_equal_single(eng, 3, 1, 6, 5, cov=False)
        d = eng.moments_rungs()                                      # the defaults: every recorded rung, all features, the whole window
        assert d[0].shape == (4, 6) and d[1].shape == (4, 6, 6) and d[3] == 70 * 40
        assert same_bits(d[1][2], eng.posterior_moments(2)[1])
        assert len({d[1][r].tobytes() for r in range(4)}) == 4       # the rungs are told apart
    finally:
        eng.close()


def test_moments_rungs_at_33_dimensions_and_with_small_groups(monkeypatch):
    eng = run_engine(33, 3, 70, 12, 1, 16, 3)
    try:
        for nfeat in (1, 6, 33):
            want = assert_rungs_equal_single(eng, 0, 3, nfeat, 7)
        monkeypatch.setenv("PTM_MOMENTS_GROUP", "64")                # two launches of the cross kernel a rung: 64 and 6 walkers
        got = eng.moments_rungs(0, 3, 33, 7)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and same_bits(got[2], want[2])
    finally:
        eng.close()


def test_moments_rungs_in_a_wrapped_ring_with_ragged_counts():
    """add_every_n = 3, five exchange candidates a step: a rung exchanged twice in a step makes an extra add_state call, so the walkers
    of the inner rungs differ in their counts and each uses its own window"""
    nt, steps, cap = 8, 900, 100
    eng = run_engine(3, nt, 70, steps, 3, cap, 4, swap_rate=0.3, seed=0x5EED0E56)
    try:
        nh = eng.nhist.reshape(nt, 70)
        assert len(set(nh[1].tolist())) >= 2 and eng.history()["row"].max() >= cap
        for nrows in (1, 5, cap):
            assert_rungs_equal_single(eng, 0, 4, 3, nrows)
        assert eng.moments_rungs()[3] == 70 * cap                    # the default window of a wrapped ring: its capacity
        out = [np.full((4, 3), -7.0), np.full((4, 3, 3), -7.0), np.full((4, 3), -7.0)]
        count = E.C.c_int64(-7)
        for first, n, nfeat, nrows in ((0, 4, 3, cap + 1), (2, 3, 3, 5), (-1, 2, 3, 5), (0, 0, 3, 5), (0, 4, 4, 5), (0, 4, 0, 5), (0, 4, 3, 0)):
            rc = eng.L.ptm_moments_rungs(eng.h, first, n, nfeat, nrows, E._d(out[0]), E._d(out[1]), E._d(out[2]), E.C.byref(count))
            assert rc == -1, (first, n, nfeat, nrows)
        with eng.batch():
            with pytest.raises(E.PtmError):
                eng.moments_rungs(0, 4, 3, 5)
        assert all((o == -7.0).all() for o in out) and count.value == -7
        assert_rungs_equal_single(eng, 0, 4, 3, 5)                   # the engine is none the worse for it
    finally:
        eng.close()


def test_one_rungs_lost_window_refuses_the_whole_call():
    """rung 0 is never exchanged twice in a step: its walkers have made exactly `steps` add_state calls, the walkers of rung 1 more.  A
    window of as many rows as every walker of rung 1 has saved is there for rung 1 and not for rung 0: the call for both is refused and
    writes nothing"""
    nt, steps = 8, 900
    eng = run_engine(3, nt, 70, steps, 1, steps + 200, 2, swap_rate=0.3, seed=0x5EED0E56)
    try:
        nh = eng.nhist.reshape(nt, 70)
        assert (nh[0] == steps).all()
        nrows = int(nh[1].min())
        assert steps < nrows <= steps + 200, nrows
        assert_rungs_equal_single(eng, 1, 1, 3, nrows)
        out = [np.full((2, 3), -7.0), np.full((2, 3, 3), -7.0), np.full((2, 3), -7.0)]
        count = E.C.c_int64(-7)
        rc = eng.L.ptm_moments_rungs(eng.h, 0, 2, 3, nrows, E._d(out[0]), E._d(out[1]), E._d(out[2]), E.C.byref(count))
        assert rc == -1 and b"fewer than nrows" in eng.L.ptm_last_error()
        assert all((o == -7.0).all() for o in out) and count.value == -7
        assert_rungs_equal_single(eng, 0, 2, 3, steps)
    finally:
        eng.close()


# ---- ptm_eigen_factors ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    g = P.golden()
    for n in P.SIZES:       # the matrices are made from the generator's normals by elementwise arithmetic: the same bits everywhere
        for kind in P.KINDS:
            assert g["%s:%d" % (kind, n)]["input"] == P.digest(P.matrix(kind, n)), ("this numpy makes other test matrices", kind, n)
    return g


def check_against_recorded(gold, kind, n, F, lam, sw, what):
    g = gold["%s:%d" % (kind, n)]
    assert P.digest(F) == g["F"], (what, kind, n, "factors")
    assert P.digest(lam) == g["lambda"], (what, kind, n, "lambda")
    assert int(sw) == g["sweeps"], (what, kind, n, "sweeps", int(sw), g["sweeps"])


@pytest.mark.parametrize("n", P.SIZES)
def test_eigen_factors_equal_the_twin(gold, n):
    """n_mat = 1 for every kind of matrix, and 300 matrices in one call (more than the chip has CUs), the kinds in turn"""
    for kind in P.KINDS:
        F, lam, sw = E.eigen_factors(P.matrix(kind, n), lambdas=True, sweeps=True)
        check_against_recorded(gold, kind, n, F, lam, sw, "one matrix")
    kinds = [P.KINDS[m % len(P.KINDS)] for m in range(300)]
    mats = {k: P.matrix(k, n) for k in P.KINDS}
    F, lam, sw = E.eigen_factors(np.stack([mats[k] for k in kinds]), lambdas=True, sweeps=True)
    assert F.shape == (300, n, n) and lam.shape == (300, n) and sw.shape == (300,)
    for m in (0, 1, 2, 3, 4, 5, 6, 7, 255, 256, 257, 292, 293, 294, 295, 296, 297, 298, 299):
        check_against_recorded(gold, kinds[m], n, F[m], lam[m], sw[m], "matrix %d of 300" % m)
    for m in range(8, 300):                                         # ... and every other one equals its kind's first
        assert P.same_bits(F[m], F[m % 8]) and P.same_bits(lam[m], lam[m % 8]) and sw[m] == sw[m % 8], (n, m)
    only = E.eigen_factors(mats["spd"])                             # without the optional outputs
    assert P.same_bits(only, F[0])


@pytest.mark.parametrize("n", [1, 2, 3, 6, 17])
def test_eigen_factors_equal_the_twin_run_here(n):
    """where the twin takes a moment it is run itself, on matrices no recorded answer exists for"""
    for seed in (1, 2):
        for kind in ("spd", "repeated", "nan", "huge"):
            Cm = P.matrix(kind, n, seed)
            F, lam, sw = E.eigen_factors(Cm, lambdas=True, sweeps=True)
            wF, wlam, wsw = P.eigen_factor(Cm)
            assert P.same_bits(F, wF) and P.same_bits(lam, wlam) and sw == wsw, (kind, n, seed)


# ---- ptm_adapt_proposals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PC.CASES))
def test_adapting_on_the_device_equals_setting_the_rungs_by_hand(name):
    print(PC.run_case(name))


def small_engine(kind=E.PROP_DENSE, D=4, Nt=3, W=8, hr=None, steps=30, configure=True, swap_rate=0.3):
    eng = E.Engine(D, Nt, W, seed=0x5EEDAD02, swap_rate=swap_rate, history_rungs=Nt if hr is None else hr, history_capacity=64)
    pr = GaussianProblem(D, Nt, 1e2)
    if configure:
        pr.configure(eng, kind)
    else:
        eng.set_bounds([E.BOUND_OPEN] * D, [E.BOUND_OPEN] * D, np.zeros(D), np.zeros(D))
        eng.set_prior(pr.types, pr.centers, pr.halfwidths)
        eng.set_target_gaussian(pr.P, pr.like0)
        eng.set_ladder(pr.beta)
    eng.init_from_prior()
    if steps and configure:
        eng.step(steps)
        eng.sync()
    return eng


def test_a_constant_parameter_keeps_the_rungs_factor():
    """rung 1's walkers all hold the same value of parameter 2 in every saved row: a zero variance, status 2, the factor stays.  A twin
    engine that never adapts, compared on that rung alone (no exchanges: the rungs do not meet)"""
    D, Nt, W = 4, 3, 8
    engines = []
    for kind in (E.PROP_DENSE, E.PROP_DIAG):
        A, B = small_engine(kind, steps=0, swap_rate=0.0), small_engine(kind, steps=0, swap_rate=0.0)
        engines += [A, B]
        for e in (A, B):
            x = e.states().reshape(Nt, W, D).copy()
            x[1, :, 2] = 0.125
            e.set_states(x.reshape(-1, D))
        # parameter 2 of rung 1 moves with a zero sigma: its factor's row (DENSE) or sigma (DIAG) is 0 there, on both engines
        for e in (A, B):
            f = np.zeros(D) if kind == E.PROP_DIAG else np.zeros((D, D))
            if kind == E.PROP_DIAG:
                f[:] = 0.01
                f[2] = 0.0
            else:
                f[np.arange(D), np.arange(D)] = 0.01
                f[2, 2] = 0.0
            e.set_proposal_rung(1, f)
            e.step(20)
            e.sync()
        assert (A.history()["x"][:, W:2 * W, 2][A.history()["row"][:, W:2 * W] >= 1] == 0.125).all()
        status, fac = A.adapt_proposals(nrows=20, factors=True)
        assert status.tolist() == [0, 2, 0], (kind, status)
        for e in (A, B):
            e.step(10)
            e.sync()
        sl = slice(W, 2 * W)
        assert same_bits(A.states()[sl], B.states()[sl]) and same_bits(A.llike[sl], B.llike[sl])
        assert np.array_equal(A.naccept[sl], B.naccept[sl]) and np.array_equal(A.last_type[sl], B.last_type[sl])
        assert not same_bits(A.states()[:W], B.states()[:W])        # ... while rung 0 took its new factor
    for e in engines:
        e.close()


def test_refusals_leave_the_engine_as_it_was():
    A, B = small_engine(), small_engine()
    try:
        st = np.full(3, -7, dtype=np.int32)
        sp = st.ctypes.data_as(E._i32p)
        call = lambda e, first, n, nrows, scale, s=sp: e.L.ptm_adapt_proposals(e.h, first, n, nrows, scale, s, None)
        INVALID, UNSUPPORTED = -1, -2
        assert call(A, 0, 3, 10, 1.0, None) == INVALID                                  # null status
        for first, n in ((-1, 2), (0, 4), (2, 2), (0, 0), (3, 1)):
            assert call(A, first, n, 10, 1.0) == INVALID, (first, n)                    # a range outside history_rungs
        for scale in (0.0, -1.0, np.inf, np.nan):
            assert call(A, 0, 3, 10, scale) == INVALID, scale
        assert call(A, 0, 3, 0, 1.0) == INVALID and call(A, 0, 3, -3, 1.0) == INVALID   # nrows < 1
        assert call(A, 0, 3, 31, 1.0) == INVALID                                        # more rows than the chains have saved
        assert call(A, 0, 3, 65, 1.0) == INVALID                                        # ... than the ring holds
        with A.batch():
            assert call(A, 0, 3, 10, 1.0) == UNSUPPORTED
        assert (st == -7).all()
        for e in (A, B):
            e.step(5)
            e.sync()
        assert same_bits(A.states(), B.states()) and np.array_equal(A.naccept, B.naccept)
        assert (A.adapt_proposals(nrows=10) == 0).all()                                 # ... and then it works
    finally:
        A.close()
        B.close()
    cases = []
    e = small_engine(configure=False)                                                   # no ptm_set_proposals yet
    cases.append((e, INVALID))
    e = small_engine(E.PROP_LOWER)
    cases.append((e, UNSUPPORTED))
    e = small_engine(hr=0)                                                              # no history ring: no range is inside it
    cases.append((e, INVALID))
    e = small_engine()
    e.set_proposal_callback(lambda X, r, w, s: (X, np.zeros(len(X)), np.zeros(len(X), dtype=np.int32), np.ones(len(X), dtype=np.int32)))
    cases.append((e, INVALID))                                                          # host-side proposals
    e = small_engine()
    never_called = E.PROPOSE_DEVICE_FN(lambda *a: None)                                 # (the engine is not stepped with it)
    e.set_proposal_device_c(E.C.cast(never_called, E.C.c_void_p))
    cases.append((e, INVALID))                                                          # device user proposals
    lone = E.Engine(4, 3, 1, seed=1, history_rungs=3, history_capacity=8)               # one walker, one row: one sample
    GaussianProblem(4, 3, 1e2).configure(lone, E.PROP_DENSE)
    lone.init_from_prior()
    lone.step(4)
    assert lone.L.ptm_adapt_proposals(lone.h, 0, 3, 1, 1.0, sp, None) == INVALID
    lone.close()
    for e, want in cases:
        try:
            assert e.L.ptm_adapt_proposals(e.h, 0, 1, 5, 1.0, sp, None) == want, want
        finally:
            e.close()
    big = E.Engine(130, 2, 2, seed=1, history_rungs=2, history_capacity=8)              # DENSE above 128 dimensions
    try:
        GaussianProblem(130, 2, 1e2).configure(big, E.PROP_DENSE)
        big.init_from_prior()
        big.step(4)
        assert big.L.ptm_adapt_proposals(big.h, 0, 2, 4, 1.0, sp, None) == UNSUPPORTED
    finally:
        big.close()
    assert (st == -7).all()


# ---- statistics -------------------------------------------------------------------------------------------------------------------
def test_adapted_rungs_keep_their_tempered_gaussians():
    """tests/test_gpu_statistics.py's form: start from exact samples of every rung's tempered Gaussian N(0, C / beta_r), record, adapt
    twice during the run, run on with fixed proposals.  Every rung keeps its covariance: the pooled estimate over the W independent
    walkers' final states has entries whose standard error is sqrt((C_ii C_jj + C_ij^2) / (beta^2 W)); that file's threshold, 5 sigma"""
    D, Nt, W = 4, 4, 4096
    pr = GaussianProblem(D, Nt, 1e1)
    eng = E.Engine(D, Nt, W, seed=0x5EEDAD03, swap_rate=0.1, history_rungs=Nt, history_capacity=32)
    try:
        pr.configure(eng, E.PROP_DENSE)
        Cov = np.linalg.inv(pr.P)
        rng = np.random.default_rng(11)
        L = np.linalg.cholesky(Cov)
        x0 = np.concatenate([(rng.standard_normal((W, D)) @ L.T) / np.sqrt(pr.beta[r]) for r in range(Nt)])
        eng.set_states(x0)
        for _ in range(2):
            eng.step(20)
            assert (eng.adapt_proposals(nrows=20) == 0).all()
        eng.step(60)
        eng.sync()
        x = eng.states().reshape(Nt, W, D)
        tries, acc = eng.ntries.reshape(Nt, W).sum(axis=1), eng.naccept.reshape(Nt, W).sum(axis=1) - W
        for r in range(Nt):
            want = Cov / pr.beta[r]
            got = x[r].T @ x[r] / W                                   # (the mean is known: 0)
            se = np.sqrt((np.outer(np.diag(want), np.diag(want)) + want ** 2) / W)
            z = np.abs(got - want) / se
            print("rung", r, "max z", z.max(), "accepted", acc[r], "of", tries[r])
            assert z.max() < 5.0, (r, z.max())
            assert 0 < acc[r] < tries[r], (r, acc[r], tries[r])
    finally:
        eng.close()
