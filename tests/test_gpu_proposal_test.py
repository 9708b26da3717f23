"""The proposal test on the device (ptmcmc_amd.engine.proposal_invariance: the reference's test_proposal::test with the engine as the
transform and exact nearest neighbours for the KL estimate): proposals that leave the target invariant pass, a contraction that
does not is told apart by orders of magnitude.  Three dimensions, one wrapped, one with a `limit` bound that cuts the target; the
runs are made by tests/proposal_test_worker.py in a child process (torch before the engine library)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest


pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
# (the worker's: it is not imported here, it imports torch)
DIM, NSAMP, NCYC, NTRY = 3, 2048, 10, 4
CENTRE, SIGMA = np.array([3.0, 0.0, -2.0]), np.array([0.4, 0.5, 2.0])


@functools.lru_cache(maxsize=None)
def runs():
    r = subprocess.run([sys.executable, os.path.join(HERE, "proposal_test_worker.py")], capture_output=True, text=True, timeout=300)   # (a few seconds: the limit only ends a hung one)
    if r.returncode < 0 or r.returncode in (134, 139):   # a crashed child (abort, fault): start nothing more on the device
        pytest.exit("proposal_test_worker.py died (exit %d)\n%s" % (r.returncode, r.stderr[-6000:]), returncode=1)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    for which, res in out.items():
        print(which, {k: v for k, v in res.items() if k not in ("target", "transformed")})
        for k in ("target", "transformed", "kl_redraws", "fake_kl_redraws"):
            res[k] = np.array(res[k])
    return out


def run(which):
    return runs()[which]


def test_the_target_samples_respect_the_space():
    r = run("native")
    t = r["target"]
    assert t.shape == (NSAMP, DIM) and (t[:, 0] >= 0).all() and (t[:, 0] < 2 * np.pi).all() and (t[:, 1] >= -0.6).all()
    assert abs(t[:, 2].mean() - CENTRE[2]) < 5 * SIGMA[2] / np.sqrt(NSAMP) and abs(t[:, 2].std() / SIGMA[2] - 1) < 5 / np.sqrt(2 * NSAMP)
    assert len(r["kl_redraws"]) == NTRY and len(r["fake_kl_redraws"]) == 30 * NTRY


@pytest.mark.parametrize("which", ["native", "device"])
def test_a_correct_proposal_is_not_told_from_the_target(which):
    """under the null the alt-transformed fake KL exceeds twice the largest of 120 redraw values for about one seed in several hundred;
    the seed is fixed"""
    r = run(which)
    assert 0 < r["acceptance"] < 1
    assert not np.array_equal(r["transformed"], r["target"])
    assert (r["transformed"][:, 1] >= -0.6).all()
    assert r["alt_fake_kl"] <= 2 * np.abs(r["fake_kl_redraws"]).max(), (r["alt_fake_kl"], np.abs(r["fake_kl_redraws"]).max())


def test_a_contraction_is_told_from_the_target():
    """after 10 cycles every variance is 0.9^20 ~ 0.12 of the target's: the fake KL against a fresh sample is of order the dimension"""
    r = run("contraction")
    assert r["acceptance"] == 1.0 and r["sweeps"] == NCYC
    assert r["alt_fake_kl"] > 100 * np.abs(r["fake_kl_redraws"]).max(), (r["alt_fake_kl"], np.abs(r["fake_kl_redraws"]).max())
    assert r["kl_verdict"] == "FAIL" and r["fake_kl_verdict"] == "FAIL"


# ---- the facade's proposal_tester and the sampler's --prop_test_index (tests/cxx/proposal_test_main.cc) ---------------------------------
ROOT = os.path.dirname(HERE)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def tester_exe(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("proposal_test")), "proposal_test")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "ptmcmc_amd", "host"), "-x", "hip", os.path.join(HERE, "cxx", "proposal_test_main.cc"),
                           "-L", os.path.join(ROOT, "ptmcmc_amd"), "-lptm_engine", "-Wl,-rpath," + os.path.join(ROOT, "ptmcmc_amd"), "-o", exe])
    return exe


def run_tester(exe, args, cwd, host_kl=False):
    env = dict(os.environ)
    env.pop("PTM_HOST_KL", None)
    if host_kl:
        env["PTM_HOST_KL"] = "1"
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300, cwd=cwd, env=env)
    if r.returncode < 0 or r.returncode in (134, 139):   # a crashed child (abort, fault): start nothing more on the device
        pytest.exit("proposal_test %s died (exit %d)\n%s" % (args, r.returncode, r.stderr[-6000:]), returncode=1)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def result_of(out):
    words = out.strip().splitlines()[-1].split()
    assert words[0] == "RESULT", out[-2000:]
    return dict(w.split("=") for w in words[1:])


REFERENCE_LINES = ("Testing proposal: ", "ncyc=10", "Applying transform:", "target mean:      ", "target var:       ", "transformed mean: ", "transformed var:  ",
                   "Computing KL divergences:", "Computing 'fake' KL divergences:", "Estimate that only 50% of KLdiff measurements are likely to exceed ",
                   "Transformed KLdiv=", "Alt-transformed KLdiv=", "Estimate that only 8.33333% of fKLdiff measurements are likely to exceed ",
                   "Transformed fKLdiv=", "Alt-transformed fKLdiv=")


@pytest.mark.parametrize("which", ["native", "device"])
def test_the_facade_tester_on_a_correct_proposal(tester_exe, tmp_path, which):
    out = run_tester(tester_exe, [which], str(tmp_path))
    print(out)
    for start in REFERENCE_LINES:
        assert any(ln.startswith(start) for ln in out.splitlines()), start
    r = result_of(out)
    assert 0 < float(r["accept"]) < 1 and r["moved"] == "1"
    assert float(r["alt_fkl"]) <= 2 * float(r["fkl_redraw_max"])
    assert run_tester(tester_exe, [which], str(tmp_path), host_kl=True) == out        # the host estimator: the same values, character for character
    if which == "native":        # the same engine, seed and arithmetic as the binding's run
        py = run("native")
        assert float(r["alt_fkl"]) == pytest.approx(py["alt_fake_kl"], rel=1e-12) and float(r["accept"]) == pytest.approx(py["acceptance"], abs=1e-6)


def test_the_facade_tester_on_a_contraction(tester_exe, tmp_path):
    out = run_tester(tester_exe, ["contraction", "./"], str(tmp_path))
    print(out)
    r = result_of(out)
    assert float(r["accept"]) == 1.0 and r["kl"] == "FAIL" and r["fkl"] == "FAIL"
    assert float(r["alt_fkl"]) > 100 * float(r["fkl_redraw_max"])
    assert out.count("FAIL\nKL value is ") == 2 and out.count(" times the stated threshold.") == 2
    assert run_tester(tester_exe, ["contraction", "./"], str(tmp_path), host_kl=True) == out
    for tag in ("target", "transformed"):       # a path was given: the two sample files, a state per line
        rows = np.loadtxt(os.path.join(str(tmp_path), "test_prop_%s.dat" % tag), delimiter=",")
        assert rows.shape == (NSAMP, DIM)


def test_hastings_err_needs_a_host_side_proposal(tester_exe, tmp_path):
    out = run_tester(tester_exe, ["native_err"], str(tmp_path))
    assert "it needs a host-side proposal" in out and out.strip().endswith("RESULT refused")
    out = run_tester(tester_exe, ["host"], str(tmp_path))           # the control: the same host-side proposal with the ratio right, 256 samples
    print(out)
    r = result_of(out)
    assert 0 < float(r["accept"]) < 1 and r["moved"] == "1" and float(r["alt_fkl"]) <= 2 * float(r["fkl_redraw_max"])
    out = run_tester(tester_exe, ["host_err"], str(tmp_path))       # 256 samples through the host-proposal step, the ratio off by 0.5
    print(out)
    r = result_of(out)
    assert r["fkl"] == "FAIL" and float(r["alt_fkl"]) > 2 * float(r["fkl_redraw_max"])


def test_a_target_at_the_seam_of_a_wrapped_dimension_is_refused_not_failed(tester_exe, tmp_path):
    """the engine wraps a Gaussian's draws and evaluates the plain Gaussian: at the seam the samples and the density differ, and a
    correct proposal would be reported FAIL"""
    out = run_tester(tester_exe, ["seam"], str(tmp_path))
    print(out)
    assert "sigma of the seam of wrapped dimension 0" in out and out.strip().endswith("RESULT refused") and "FAIL" not in out


def test_the_sampler_moves_a_test_distribution_in_from_the_seam(tester_exe, tmp_path):
    """the prior of the wrapped dimension is [0.05, 0.35] on [0, 2 pi): every centre the sampler draws lies within a few of its sigmas
    of the seam.  It is moved 6 sigma in, and the correct proposal (the run's Gaussian set) passes: fixed seed; under the null the
    fake KL exceeds its 8.3 % cut for about one seed in twelve -- if this seed is one, change it and say so here."""
    out = run_tester(tester_exe, ["sampler_wrap", "run", "--seed=0.25", "--prop_test_index=."], str(tmp_path))
    head = out.split("Running chain")[0]
    print(head[-3000:])
    assert "Wrapped dimension 0: centre " in head and " moved 6 sigma in from the seam." in head
    assert "Testing on 2048 samples, applying proposal through 10 cycles and calibrating with 4 trials." in head
    assert "sigma of the seam" not in head           # the tester had nothing to refuse
    verdicts = [ln for ln in head.splitlines() if ln in ("PASS", "FAIL")]
    assert len(verdicts) == 2 and verdicts[1] == "PASS", verdicts        # (KL, fake KL)


def test_the_samplers_flag_tests_and_leaves_the_run_alone(tester_exe, tmp_path):
    dirs = {}
    for name, flags in (("plain", []), ("whole", ["--prop_test_index=."]), ("members", ["--prop_test_index=L"])):
        dirs[name] = os.path.join(str(tmp_path), name)
        os.mkdir(dirs[name])
        out = run_tester(tester_exe, ["sampler", "run"] + flags, dirs[name])
        if name == "plain":
            assert "Testing proposal" not in out
            continue
        print(out[:6000])
        for start in ("Checking limits: ", "Test distribution is: ", "Testing on 512 samples, applying proposal through 5 cycles and calibrating with 2 trials.",
                      "path='./test_prop'", "Estimate that only 50% of KLdiff measurements are likely to exceed ",
                      "Estimate that only 11.6667% of fKLdiff measurements are likely to exceed "):
            assert any(ln.startswith(start) for ln in out.splitlines()), start
        assert out.count("Testing proposal: ") == (1 if name == "whole" else 7) and ("6 members in proposal set" in out) == (name == "members")
        files = sorted(f for f in os.listdir(dirs["plain"]) if f.startswith("run") and f.endswith(".dat"))
        assert files
        for f in files:      # the chain files of the run that follows are those of a run without the flag
            assert open(os.path.join(dirs[name], f), "rb").read() == open(os.path.join(dirs["plain"], f), "rb").read(), f
