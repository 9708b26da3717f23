"""The statistics of the proposal test without a device: the recorded answers of the real reference (tests/golden/kl_divergence.json.gz:
test_proposal.hh's KL_divergence with exact neighbours, its two distance arrays, fake_KL_divergence) against the Python twin
(tests/kl_model.py), the facade's kl_estimator (tests/cxx/kl_fixture_main.cc) and the binding's host-side halves; the named wrong
readings; the cut and the verdict of the test on fed-in values."""
import math
import tempfile

import numpy as np
import pytest

import kl_model as K
from ptmcmc_amd import engine as E

CASES = [c["name"] for c in K.load()["cases"]]


def case(name):
    return next(c for c in K.load()["cases"] if c["name"] == name)


@pytest.fixture(scope="module")
def fixture_exe():
    with tempfile.TemporaryDirectory() as d:
        yield K.build_fixture_driver(d)


@pytest.fixture(scope="module")
def facade_answers(fixture_exe):
    cases = K.load()["cases"]
    return dict(zip(CASES, K.parse_sets_output(K.run_driver(fixture_exe, K.sets_input(cases)))))


def test_the_fixture_covers_what_it_must():
    cases = K.load()["cases"]
    assert {c["dim"] for c in cases} == {1, 2, 5}
    sizes = [len(c["P"]) for c in cases]
    assert min(sizes) == 7 and max(sizes) == 200 and any(len(c["P"]) != len(c["Q"]) for c in cases)
    assert any(np.array_equal(c["P"] - (c["P"][0] - c["Q"][0]), c["Q"]) for c in cases if len(c["P"]) == len(c["Q"]))     # P = shifted Q
    assert any(0.0 in c["r1sqs"] for c in cases)                                                                          # duplicates: the floor acts
    for c in cases:      # a wrapped dimension in which the alternative distance wins for some pairs
        if any(c["wrapped"]):
            assert not K.same_bits(K.pair_dist2(c["P"], c["Q"], *c["bounds"]), K.pair_dist2(c["P"], c["Q"], *c["bounds"], wrap_alternative=False))
    assert sum(any(c["wrapped"]) for c in cases) >= 2


@pytest.mark.parametrize("name", CASES)
def test_the_twin_reproduces_the_reference_bit_for_bit(name):
    c = case(name)
    value, r, s = K.kl(c["P"], c["Q"], *c["bounds"], detail=True)
    assert K.same_bits(r, c["r1sqs"]) and K.same_bits(s, c["s1sqs"])
    assert K.same_bits(value, c["kl"]), (value, c["kl"])
    assert K.same_bits(E.kl_from_distances(r, s, c["dim"], len(c["Q"])), c["kl"])         # the binding's floor and sum


@pytest.mark.parametrize("name", CASES)
def test_the_facade_estimator_reproduces_the_reference_bit_for_bit(facade_answers, name):
    c, got = case(name), facade_answers[name]
    assert K.same_bits(got["r"], c["r1sqs"]) and K.same_bits(got["s"], c["s1sqs"])
    assert K.same_bits(got["kl"], c["kl"]), (got["kl"], c["kl"])


def test_fake_kl_agrees_with_the_reference_relatively(facade_answers):
    """another matrix inverse than Eigen's: the largest relative difference measured when the fixture was written stands in its header;
    ten times that is allowed for a different compiler's rounding of the same formula"""
    fx = K.load()
    measured, smallest = fx["fake_kl_model_max_rel_diff"], fx["fake_kl_smallest_abs"]
    assert 0 < measured < 1e-12 and fx["fake_kl_model_max_abs_diff"] < 1e-9 * smallest      # small against the smallest |fake KL|
    assert smallest == min(abs(c["fake_kl"]) for c in fx["cases"])
    for c in fx["cases"]:
        for who, got in (("twin", K.fake_kl(c["P"], c["Q"])), ("facade", facade_answers[c["name"]]["fkl"]), ("binding", E.fake_kl_divergence(c["P"], c["Q"]))):
            rel = abs(got - c["fake_kl"]) / abs(c["fake_kl"])
            print(c["name"], who, got, c["fake_kl"], rel)
            assert rel <= 10 * measured, (c["name"], who, got, c["fake_kl"])


@pytest.mark.parametrize("wrong", sorted(K.WRONG))
def test_a_named_wrong_reading_misses_a_recorded_answer(wrong):
    missed = [c["name"] for c in K.load()["cases"] if not K.same_bits(K.kl(c["P"], c["Q"], *c["bounds"], **K.WRONG[wrong]), c["kl"])]
    print(wrong, missed)
    assert missed


def test_too_few_samples_are_refused():
    x = np.arange(12.0).reshape(6, 2)
    with pytest.raises(ValueError):
        K.kl(x, x + 0.5)
    with pytest.raises(ValueError):
        E.kl_from_distances(np.ones(6), np.ones(6), 2, 6)
    with pytest.raises(ValueError):
        E.kl_divergence(x, x + 0.5)           # (refused before the device is asked)


@pytest.mark.parametrize("ntry", [2, 10, 20])
def test_the_cut_and_the_verdict_follow_the_reference(fixture_exe, ntry):
    rng = np.random.default_rng(ntry)
    diffs = rng.standard_normal(ntry) * 0.01
    ncut, frac, cut, _ = K.verdict(diffs, 0.0)
    assert ncut == {2: 1, 10: 3, 20: 4}[ntry] and frac == ncut / ntry
    d = np.sort(np.abs(diffs))
    assert cut == (d[ntry - ncut] + d[ntry - ncut - 1]) / 2.0
    for alt, transformed in ((0.5 * cut, 0.4 * cut), (3.0 * cut, 0.1 * cut), (-1.0, 0.0)):
        want = K.verdict(diffs, alt)
        assert want[3] == (alt < cut)
        text = "verdict fKL 5 %d %.17g %.17g %.17g %.17g\n%s\n" % (ntry, transformed, 0.25, alt, 0.125, " ".join("%.17g" % v for v in diffs))
        lines = K.run_driver(fixture_exe, text).splitlines()
        head = lines[0].split()
        assert (int(head[1]), float(head[2]), float(head[3]), bool(int(head[4]))) == want
        assert lines[1] == "" and lines[2].startswith("Estimate that only %g%% of fKLdiff measurements are likely to exceed " % (frac * 100))
        assert lines[2].endswith(" for matching distributions.")
        assert lines[3].startswith("Transformed fKLdiv=") and lines[3].endswith(" <-> 0.25")
        assert lines[4].startswith("Alt-transformed fKLdiv=") and lines[4].endswith(" <-> 0.125")
        small = alt - transformed > abs(cut)
        assert lines[5].startswith("When 'Transformed' is signficantly less than 'alt-Transformed'") == small
        rest = lines[5 + small:]
        assert rest == ["PASS"] if want[3] else (rest[0] == "FAIL" and rest[1].startswith("KL value is ") and rest[1].endswith(" times the stated threshold."))


def test_one_redraw_gives_no_cut(fixture_exe):
    assert K.verdict([0.3], -0.1) == (1, 1.0, 0.0, True)
    lines = K.run_driver(fixture_exe, "verdict KL 5 1 0.1 0.1 0.2 0.2\n0.3\n").splitlines()
    assert lines[0].split()[1:] == ["1", "1", "0", "0"] and lines[1].startswith("Transformed KLdiv=") and "FAIL" in lines
    assert not any(ln.startswith("Estimate") for ln in lines) and math.isinf(float(lines[-1].split()[3]))


def test_a_wrapped_target_at_its_seam_is_refused_before_any_engine_is_built():
    """the engine wraps a Gaussian's draws but evaluates the plain Gaussian: within SEAM_SIGMAS sigma of the seam the test would be wrong"""
    bounds = ([E.BOUND_WRAP, E.BOUND_OPEN], [E.BOUND_WRAP, E.BOUND_OPEN], [0.0, 0.0], [2 * np.pi, 0.0])
    for centre, sigma in (([0.5, 0.0], [0.4, 1.0]), ([6.0, 0.0], [0.1, 1.0]), ([3.0, 0.0], [0.6, 1.0])):
        with pytest.raises(ValueError, match="seam of wrapped dimension 0"):
            E.proposal_invariance(2, centre, sigma, lambda eng: None, nsamp=64, bounds=bounds)
