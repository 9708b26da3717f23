"""Proposal factors from a covariance without a device: the Python twin (tests/prop_adapt_model.py) of the facade's
gaussian_prop::eigen_factor against the facade itself (tests/cxx/prop_adapt_main.cc, bit for bit, also built under the address and
undefined-behaviour sanitizers as a stand-alone host program), against its recorded answers (tests/golden/prop_adapt_hashes.json, which
stand for the twin in the device tests where running it takes minutes), a reconstruction bound, deliberate misreadings that the
comparison must tell apart, the status rule, and the C ABI's declarations, exports and early refusals."""
import ctypes as C
import os
import re
import tempfile

import numpy as np
import pytest

import prop_adapt_model as P
from ptmcmc_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(k, n) for n in P.SIZES for k in P.KINDS]
# max |F F^T - C| of the twin over the symmetric positive definite test matrices (random, identity, descending diagonal, repeated
# eigenvalues; all sizes), measured on the CPU: RECONSTRUCTION_WORST, at 128 dimensions with repeated eigenvalues.  Four times that is
# allowed (5.42e-12): the check is there to catch a wrong rotation, not to grade Jacobi.
RECONSTRUCTION_WORST = 1.3558043576722412e-12
RECONSTRUCTION_BOUND = 4 * RECONSTRUCTION_WORST
RECONSTRUCTION_KINDS = ("spd", "identity", "descending", "repeated")


@pytest.fixture(scope="module")
def facade_answers():
    with tempfile.TemporaryDirectory() as d:
        exe = P.build_fixture_driver(d)
        got = P.fixture_driver_answers(exe, [P.matrix(k, n) for k, n in CASES])
    return dict(zip(CASES, got))


@pytest.mark.parametrize("n", P.SIZES)
def test_the_facade_and_the_twin_agree_bit_for_bit(facade_answers, n):
    for kind in P.KINDS:
        _, F, lam, _, _ = P.reference(kind, n)
        gF, glam = facade_answers[(kind, n)]
        assert P.same_bits(gF, F), (kind, n, "F")
        assert P.same_bits(glam, lam), (kind, n, "lambda")


@pytest.mark.parametrize("n", P.SIZES)
def test_the_twin_gives_its_recorded_answers(n):
    gold = P.golden()
    for kind in P.KINDS:
        assert gold["%s:%d" % (kind, n)] == P.record(kind, n), (kind, n)


def test_the_facade_code_under_the_sanitizers():
    """the same program built with -fsanitize=address,undefined: a finding ends it with a non-zero status"""
    cases = [(k, n) for k, n in CASES if n <= 33 or k in ("spd", "nan")]
    with tempfile.TemporaryDirectory() as d:
        exe = P.build_fixture_driver(d, sanitize=True)
        got = P.fixture_driver_answers(exe, [P.matrix(k, n) for k, n in cases])
    for (kind, n), (gF, glam) in zip(cases, got):
        _, F, lam, _, _ = P.reference(kind, n)
        assert P.same_bits(gF, F) and P.same_bits(glam, lam), (kind, n)


def test_the_factor_reconstructs_the_covariance():
    worst = 0.0
    for n in P.SIZES:
        for kind in RECONSTRUCTION_KINDS:
            Cm, F, _, _, _ = P.reference(kind, n)
            err = np.abs(F @ F.T - Cm).max()
            worst = max(worst, err)
            assert err <= RECONSTRUCTION_BOUND, (kind, n, err)
    print("worst max|F F^T - C| = %.3g (bound %.3g)" % (worst, RECONSTRUCTION_BOUND))


def test_the_matrices_exercise_what_they_are_there_for():
    for n in P.SIZES:
        assert P.reference("identity", n)[3] == 0 and P.reference("descending", n)[3] == 0 and P.reference("tiny_off", n)[3] == 0   # no sweep rotates
        lam = P.reference("descending", n)[2]
        assert (np.diff(lam) > 0).all() and lam[0] == 0.75                      # the sort acted
        assert ((P.reference("tiny_off", n)[1] != 0).sum(axis=0) == 1).all()    # skipped: F is the diagonal's roots, in sorted columns
        assert P.reference("spd", n)[4] == 0 and P.reference("repeated", n)[4] == 0 and P.reference("huge", n)[4] == 0
        assert P.reference("rank", n)[4] == 2 and not P.reference("rank", n)[2][0] > 0    # a lambda clipped at 0
        assert P.reference("nan", n)[4] == 1 and np.isnan(P.reference("nan", n)[2]).any()
        if n > 1:
            lam = P.reference("repeated", n)[2]
            assert np.allclose(lam[:n - n // 2], 1.0, atol=1e-9) and np.allclose(lam[n - n // 2:], 3.0, atol=1e-9)
            assert P.reference("huge", n)[3] >= 1 and np.isfinite(P.reference("huge", n)[1]).all()
            assert np.isnan(P.reference("nan", n)[1]).all() and P.reference("nan", n)[3] == P.SWEEPS_MAX


def test_status_rule():
    assert P.diag_status(np.array([1.0, 2.0])) == 0 and P.diag_status(np.array([1.0, 0.0])) == 2 and P.diag_status(np.array([-1.0, 2.0])) == 2
    assert P.diag_status(np.array([np.inf, 0.0])) == 1 and P.diag_status(np.array([1.0, np.nan])) == 1
    f, st = P.adapt(np.array([4.0, 9.0]), 0.5, diag=True)
    assert st == 0 and f.tolist() == [1.0, 1.5]
    Cm = P.matrix("spd", 6)
    f, st = P.adapt(Cm, 0.25)
    assert st == 0 and P.same_bits(f, 0.25 * P.reference("spd", 6)[1])
    inf = Cm.copy()
    inf[2, 3] = inf[3, 2] = np.inf
    assert P.adapt(inf, 1.0)[1] == 1


def changed(kind, n, variant):
    Cm, F, lam, sw, _ = P.reference(kind, n)
    F2, lam2, sw2 = P.eigen_factor(Cm, variant, done=None if variant == "rows_first" else P.reference_rotations(kind, n))
    return not (P.same_bits(F, F2) and P.same_bits(lam, lam2) and sw == sw2)


def test_misreadings_change_the_answers():
    """each deliberate misreading of the facade's code changes at least one output bit on at least half of the matrices it can change, so
    the device comparison cannot pass by accident.  The row loop before the column loop and the sort left out: the random symmetric
    positive definite matrices.  sqrt(lambda) unclipped: the rank n - 1 matrices -- on a positive definite matrix every lambda is above
    0, the clip never acts and leaving it out can change no bit."""
    for variant, kind in (("rows_first", "spd"), ("no_sort", "spd"), ("unclipped", "rank")):
        n_changed = sum(changed(kind, n, variant) for n in P.SIZES)
        print(variant, kind, n_changed, "of", len(P.SIZES))
        assert 2 * n_changed >= len(P.SIZES), (variant, n_changed)
    assert not any(changed("spd", n, "unclipped") for n in P.SIZES)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptm_engine.h")).read(), flags=re.S)
    lib = C.CDLL(E.LIB_PATH)
    for name in ("ptm_moments_rungs", "ptm_eigen_factors", "ptm_adapt_proposals"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(lib, name), name
        assert name in E.EXPORTS
    assert hasattr(E.Engine, "moments_rungs") and hasattr(E.Engine, "adapt_proposals") and callable(E.eigen_factors)


def test_bad_arguments_are_refused_before_a_device_is_touched():
    L = E.load()
    cov, fac = np.eye(3), np.full((3, 3), -7.0)
    st = np.full(2, -7, dtype=np.int32)
    assert L.ptm_eigen_factors(-1, None, 1, 3, E._d(fac), None, None) == -1 and b"null argument" in L.ptm_last_error()
    assert L.ptm_eigen_factors(-1, E._d(cov), 1, 3, None, None, None) == -1 and b"null argument" in L.ptm_last_error()
    for n_mat, n in ((1, 0), (1, 129), (0, 3), (-1, 3)):
        assert L.ptm_eigen_factors(-1, E._d(cov), n_mat, n, E._d(fac), None, None) == -1, (n_mat, n)
    assert L.ptm_moments_rungs(None, 0, 1, 3, 2, E._d(fac), None, None, None) == -1 and b"null argument" in L.ptm_last_error()
    assert L.ptm_adapt_proposals(None, 0, 2, 5, 1.0, st.ctypes.data_as(E._i32p), None) == -1 and b"null argument" in L.ptm_last_error()
    assert (fac == -7).all() and (st == -7).all()
    with pytest.raises(E.PtmError):
        E.eigen_factors(np.zeros((2, 3)))
