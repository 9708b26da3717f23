"""The facade's exact posterior quantiles (tests/cxx/quantiles_device_main.cc): parallel_tempering_chains::posterior_quantiles selects
from the device's own ring -- the same %.17g values as the host estimator (PTM_HOST_QUANTILES=1), the device path taken only
without it.  The sampler's --quantiles_out writes the cold rung's quantiles to a file and says so in one line
(tests/cxx/quantiles_sampler_main.cc); the medians of its Gaussian target lie where they must; without the flag the chain files are
those of the commit before the flags (tests/golden/sampler_chain_files.json.gz)."""
import gzip
import importlib.util
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import quantiles_model as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ptmcmc_amd", "host"), "-L", os.path.join(ROOT, "ptmcmc_amd"), "-lptm_engine",
         "-Wl,-rpath," + os.path.join(ROOT, "ptmcmc_amd"), "-pthread"]
QUANTILES_LINE = re.compile(r"^Posterior quantiles over (\d+) replicas, (\d+) rows: (\d+) parameters at (\d+) probabilities \((device|host)\), written to (\S+)$")

pytestmark = pytest.mark.gpu


def run(exe, args, host=False, timeout=300, expect=0):
    env = dict(os.environ)
    env.pop("PTM_HOST_QUANTILES", None)
    if host:
        env["PTM_HOST_QUANTILES"] = "1"
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == expect, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def build(d, name, source):
    exe = os.path.join(d, name)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "cxx", source)] + FLAGS + ["-o", exe])
    return exe


@pytest.fixture(scope="module")
def quantiles_device():
    with tempfile.TemporaryDirectory() as d:
        yield build(d, "quantilesdev", "quantiles_device_main.cc")


@pytest.fixture(scope="module")
def sampler():
    with tempfile.TemporaryDirectory() as d:
        yield build(d, "quantilessampler", "quantiles_sampler_main.cc"), d


@pytest.mark.parametrize("ladder", ["one", "many"])
def test_facade_gives_the_same_quantiles_from_the_device_and_from_the_host_estimator(quantiles_device, ladder):
    args = ["2000"] + (["many"] if ladder == "many" else [])
    dev, host = (run(quantiles_device, args, host=h) for h in (False, True))
    print("\n".join(dev))
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
    assert strip(dev) == strip(host)                                 # every %.17g value: quantiles and brackets
    assert len([l for l in dev if l.startswith("q ")]) == 4 * 7
    q0 = np.array([[float(v) for v in l.split()[3:]] for l in dev if l.startswith("q 0 ")])
    assert q0.shape == (7, 3) and (q0[3] <= q0[6]).all() and (q0[6] <= q0[0]).all() and (q0[0] < q0[1]).all() and (q0[1] < q0[2]).all() and (q0[2] <= q0[4]).all()
    assert q0[1].tobytes() == q0[5].tobytes() and np.abs(q0[1]).max() < 1.0


def test_host_side_proposals_use_the_host_estimator(quantiles_device):
    out = run(quantiles_device, ["1000", "hostprop"])
    queries = [l for l in out if l.startswith("query")]
    assert len(queries) == 4 and all(l.endswith("device=0") for l in queries)
    q0 = np.array([[float(v) for v in l.split()[3:]] for l in out if l.startswith("q 0 ")])
    assert q0.shape == (7, 3) and (q0[0] < q0[1]).all() and (q0[1] < q0[2]).all()


def test_sampler_writes_the_quantile_file_and_its_medians_are_the_targets(sampler):
    exe, d = sampler
    common = ["--replicas=70", "--nsteps=4000", "--nevery=1000"]
    path = os.path.join(d, "posterior.quantiles")
    out = run(exe, [os.path.join(d, "first")] + common + ["--quantiles_out=" + path])
    lines = [QUANTILES_LINE.match(l) for l in out if l.startswith("Posterior quantiles")]
    assert len(lines) == 1 and lines[0], [l for l in out if "quantiles" in l]
    nrep, nrows, npar, nprob, where, written = lines[0].groups()
    assert int(nrep) == 70 and int(npar) == 3 and int(nprob) == 3 and where == "device" and written == path and int(nrows) >= 100
    # the file's values are the engine's own answer for the same rung, window and probabilities, to the bit
    words, names, q = Q.parse_file(path)
    head = " ".join(words)
    assert "dim 3" in head and "N %d" % (70 * int(nrows)) in head and "replicas 70 x rows %s" % nrows in head and words[-4:] == ["probs", "0.050000000000000003", "0.5", "0.94999999999999996"]
    assert names == ["a", "b", "c"] and q.shape == (3, 3)
    eng = [l.split() for l in out if l.startswith("engine")]
    assert eng[0] == ["engine", str(70 * int(nrows)), nrows]
    assert q.tobytes() == np.array([[float(v) for v in l[1:]] for l in eng[1:]]).tobytes()
    # the medians of the Gaussian target lie within 5 standard errors of its mean, 0: the standard error of a Gaussian's sample
    # median, sqrt(pi / 2) sigma / sqrt(ess), with the effective samples the run's own estimator finds in the window
    ess_line = [l.split() for l in out if l.startswith("ess ")]
    ess, counted = float(ess_line[0][1]), int(ess_line[0][2])
    sigma = np.sqrt(np.diagonal(np.linalg.inv(np.array([[2.0, 0.6, 0.0], [0.6, 1.0, -0.3], [0.0, -0.3, 1.5]]))))
    se = np.sqrt(np.pi / 2) * sigma / np.sqrt(ess)
    print("medians", q[1], "standard errors", se, "ess", ess, "of", counted, "replicas; 5% and 95%", q[0], q[2], "target", -1.6449 * sigma, 1.6449 * sigma)
    assert counted == 70 and 70 <= ess <= 70 * int(nrows) * 2
    assert (np.abs(q[1]) <= 5 * se).all()
    assert (q[0] < q[1]).all() and (q[1] < q[2]).all()
    # the host estimator writes the same file
    path_h = os.path.join(d, "posterior_host.quantiles")
    out_h = run(exe, [os.path.join(d, "firsth")] + common + ["--quantiles_out=" + path_h], host=True)
    assert [QUANTILES_LINE.match(l).group(5) for l in out_h if l.startswith("Posterior quantiles")] == ["host"]
    assert open(path_h).read() == open(path).read()
    # other probabilities; a bad list is refused before anything runs
    path2 = os.path.join(d, "other.quantiles")
    out2 = run(exe, [os.path.join(d, "second"), "--replicas=70", "--nsteps=400", "--nevery=200", "--quantiles_out=" + path2, "--quantile_probs=0.5,0,1,0.25"])
    assert [QUANTILES_LINE.match(l).group(4) for l in out2 if l.startswith("Posterior quantiles")] == ["4"]
    _, _, q2 = Q.parse_file(path2)
    assert q2.shape == (4, 3) and (q2[1] <= q2[3]).all() and (q2[3] <= q2[0]).all() and (q2[0] <= q2[2]).all()
    for bad in ("0.5,1.5", "0.5,,0.7", "abc", "0.5,"):
        out3 = run(exe, [os.path.join(d, "third"), "--replicas=70", "--nsteps=400", "--quantiles_out=" + path2, "--quantile_probs=" + bad], expect=1)
        assert any("--quantile_probs" in l for l in out3) and not any(l.startswith("chain 0 step") for l in out3), bad


def test_without_the_flag_the_chain_files_are_those_of_the_commit_before():
    spec = importlib.util.spec_from_file_location("moments_probe", os.path.join(ROOT, "tools", "moments_probe.py"))
    probe = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    with gzip.open(os.path.join(ROOT, "tests", "golden", "sampler_chain_files.json.gz")) as f:
        want = json.loads(f.read().decode())
    assert want["args"] == probe.RECORD_ARGS and len(want["files"]) == 6
    got = probe.sampler_record()
    assert got["proposal"] == want["proposal"]
    assert sorted(got["files"]) == sorted(want["files"])
    for name in want["files"]:
        assert got["files"][name] == want["files"][name], name
    assert not any("quantile" in l.lower() for l in got["stdout"])
