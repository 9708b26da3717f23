"""The facade's pooled posterior moments (tests/cxx/moments_device_main.cc): parallel_tempering_chains::posterior_moments estimates
from the device's own ring -- the same %.17g values as the host estimator (PTM_HOST_MOMENTS=1), the device path taken only without
it.  The sampler's --covariance_out writes the cold rung's moments to a file that --covariance_file of a second run reads and
proposes with (tests/cxx/moments_sampler_main.cc); without either flag the chain files are those of the commit before the flags
(tests/golden/sampler_chain_files.json.gz, recorded with tools/moments_probe.py --record)."""
import gzip
import importlib.util
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import moments_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ptmcmc_amd", "host"), "-L", os.path.join(ROOT, "ptmcmc_amd"), "-lptm_engine",
         "-Wl,-rpath," + os.path.join(ROOT, "ptmcmc_amd"), "-pthread"]
MOMENTS_LINE = re.compile(r"^Posterior moments over (\d+) replicas, (\d+) rows: (\d+) parameters, standard deviations (\S+) \.\. (\S+) \((device|host)\), written to (\S+)$")

pytestmark = pytest.mark.gpu


def run(exe, args, host=False, timeout=300, expect=0):
    env = dict(os.environ)
    env.pop("PTM_HOST_MOMENTS", None)
    if host:
        env["PTM_HOST_MOMENTS"] = "1"
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == expect, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def build(d, name, source):
    exe = os.path.join(d, name)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "cxx", source)] + FLAGS + ["-o", exe])
    return exe


@pytest.fixture(scope="module")
def moments_device():
    with tempfile.TemporaryDirectory() as d:
        yield build(d, "momentsdev", "moments_device_main.cc")


@pytest.fixture(scope="module")
def sampler():
    with tempfile.TemporaryDirectory() as d:
        yield build(d, "momentssampler", "moments_sampler_main.cc"), d


@pytest.mark.parametrize("ladder", ["one", "many"])
def test_facade_gives_the_same_moments_from_the_device_and_from_the_host_estimator(moments_device, ladder):
    args = ["2000"] + (["many"] if ladder == "many" else [])
    dev, host = (run(moments_device, args, host=h) for h in (False, True))
    print("\n".join(l for l in dev if not l.startswith("walker")))
    counts = dev[0].split()
    assert counts[0] == "counts" and len(counts) == 71
    if ladder == "many":
        assert len(set(counts[1:])) >= 2                             # the replicas' windows on rung 1 are not the same rows
    queries = {w: [l for l in out if l.startswith("query")] for w, out in (("dev", dev), ("host", host))}
    assert len(queries["dev"]) == 4
    assert all(l.endswith("device=1") for l in queries["dev"]) and all(l.endswith("device=0") for l in queries["host"])
    got = [int(l.split()[5].split("=")[1]) for l in queries["dev"]]
    assert got[:2] == [35000, 17500] and got[3] == 70 and (got[2] == 70000 if ladder == "one" else got[2] >= 70000)
    strip = lambda out: [l.split(" device=")[0] for l in out]
    assert strip(dev) == strip(host)                                 # every %.17g value: means, variances, matrices, walkers' sums
    assert len([l for l in dev if l.startswith("cov")]) == 3 + 2 + 3 + 1 and len([l for l in dev if l.startswith("walker")]) == 4 * 70
    var = [float(v) for l in dev if l.startswith("var") for v in l.split()[2:]]
    assert len(var) == 9 and all(0.05 < v < 400 for v in var), var


def test_host_side_proposals_use_the_host_estimator(moments_device):
    out = run(moments_device, ["1000", "hostprop"])
    queries = [l for l in out if l.startswith("query")]
    assert len(queries) == 4 and all(l.endswith("device=0") for l in queries)
    var = [float(v) for l in out if l.startswith("var") for v in l.split()[2:]]
    assert len(var) == 9 and all(0.05 < v < 400 for v in var), var


def test_sampler_writes_the_covariance_file_and_a_second_run_proposes_with_it(sampler):
    exe, d = sampler
    common = ["--replicas=70", "--nsteps=1000", "--nevery=500"]
    path = os.path.join(d, "posterior.cov")
    out = run(exe, [os.path.join(d, "first")] + common + ["--covariance_out=" + path])
    lines = [MOMENTS_LINE.match(l) for l in out if l.startswith("Posterior moments")]
    assert len(lines) == 1 and lines[0], [l for l in out if "moments" in l]
    nrep, nrows, npar, smin, smax, where, written = lines[0].groups()
    assert int(nrep) == 70 and int(npar) == 3 and where == "device" and written == path and 0 < float(smin) <= float(smax) < 20
    assert not any("covariance_file" in l for l in out)
    # the file's matrix is the engine's own answer for the same rung and window, to the bit
    head = [l for l in open(path) if l.startswith("#")]
    assert "dim 3" in head[0] and "N %d" % (70 * int(nrows)) in head[0] and "replicas 70 x rows %s" % nrows in head[0] and head[1].split()[-3:] == ["a", "b", "c"]
    mean, cov = M.parse_file(path)
    eng = [l.split() for l in out if l.startswith("engine")]
    assert eng[0] == ["engine", str(70 * int(nrows)), nrows] and int(nrows) >= 100
    assert mean.tobytes() == np.array([float(v) for v in eng[1][1:]]).tobytes()
    assert cov.tobytes() == np.array([[float(v) for v in l[1:]] for l in eng[2:]]).tobytes()
    # the target's covariance is the inverse of its precision; a run this short, a prior box 40 wide behind it, is held to its order
    # of magnitude only (a factor 3 either way): the bits are checked above
    target = np.linalg.inv(np.array([[2.0, 0.6, 0.0], [0.6, 1.0, -0.3], [0.0, -0.3, 1.5]]))
    print(cov, target, sep="\n")
    ratio = np.diagonal(cov) / np.diagonal(target)
    assert np.all(ratio > 1 / 3.0) and np.all(ratio < 3.0) and np.all(np.linalg.eigvalsh(cov) > 0)
    # the host estimator writes the same file
    path_h = os.path.join(d, "posterior_host.cov")
    out_h = run(exe, [os.path.join(d, "firsth")] + common + ["--covariance_out=" + path_h], host=True)
    assert [MOMENTS_LINE.match(l).group(6) for l in out_h if l.startswith("Posterior moments")] == ["host"]
    strip = lambda p: [l for l in open(p) if not l.startswith("#")]
    assert strip(path_h) == strip(path)
    # a second run proposes with it: the covariance Gaussian stands in the set, behind the differential evolution, with its share
    out2 = run(exe, [os.path.join(d, "second")] + common + ["--covariance_file=" + path, "--cov_draw_frac=0.25"])
    a = out2.index("Proposal distribution is:")
    shown = "\n".join(out2[a:a + 40])
    print(shown)
    plain = "\n".join(out[out.index("Proposal distribution is:"):][:40])
    assert re.search(r"^\s*25% : StepByCovar\[dim=3\]\(1Dfrac=0.5\)$", shown, re.M) and "StepByCovar" not in plain
    assert re.search(r"^ChooseFrom\(\s*55% : DifferentialEvolution", shown, re.M) and re.search(r"^ChooseFrom\(\s*80% : DifferentialEvolution", plain, re.M)
    assert shown.count("StepBy[dim=3]") == plain.count("StepBy[dim=3]") == 6
    assert shown.index("DifferentialEvolution") < shown.index("StepByCovar") < shown.index("StepBy[dim=3]")
    assert any(l.startswith("Finished running chain 0.") for l in out2)
    assert [int(l.split("step")[1]) for l in out2 if l.startswith("chain 0 step")][-1] == 1000
    assert not any("is not read" in l for l in out + out2)
    # a file of another dimension is refused before anything runs
    bad = os.path.join(d, "bad.cov")
    open(bad, "w").write("1 2\n1 0\n0 1\n")
    out3 = run(exe, [os.path.join(d, "third")] + common + ["--covariance_file=" + bad], expect=1)
    assert any(l.startswith("read_covariance:") for l in out3) and not any(l.startswith("chain 0 step") for l in out3)


def test_without_the_flags_the_chain_files_are_those_of_the_commit_before():
    spec = importlib.util.spec_from_file_location("moments_probe", os.path.join(ROOT, "tools", "moments_probe.py"))
    probe = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    with gzip.open(os.path.join(ROOT, "tests", "golden", "sampler_chain_files.json.gz")) as f:
        want = json.loads(f.read().decode())
    assert want["args"] == probe.RECORD_ARGS and len(want["files"]) == 6 and all(len(v) > 1000 for v in want["files"].values())
    got = probe.sampler_record()
    assert got["proposal"] == want["proposal"]
    assert sorted(got["files"]) == sorted(want["files"])
    for name in want["files"]:
        assert got["files"][name] == want["files"][name], name
    assert not any("covariance" in l.lower() or "Posterior moments" in l for l in got["stdout"])
