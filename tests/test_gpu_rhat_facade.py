"""The facade's split R-hat (tests/cxx/rhat_device_main.cc): parallel_tempering_chains::split_rhat estimates from the device's own
ring -- the same %.17g values as the host estimator (PTM_HOST_RHAT=1), the device path taken only without it -- and the sampler's
--chain_rhat_stop prints and stops on the largest split R-hat of the cold chains across the replicas."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ptmcmc_amd", "host"), "-L", os.path.join(ROOT, "ptmcmc_amd"), "-lptm_engine",
         "-Wl,-rpath," + os.path.join(ROOT, "ptmcmc_amd"), "-pthread"]
RHAT_LINE = re.compile(r"^Split R-hat over (\d+) replicas, (\d+) rows: max=(\S+) \(par (\d+)\)$")


def run(exe, args, host=False, timeout=300):
    env = dict(os.environ)
    env.pop("PTM_HOST_RHAT", None)
    if host:
        env["PTM_HOST_RHAT"] = "1"
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def rhat_device():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "rhatdev")
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "cxx", "rhat_device_main.cc")] + FLAGS + ["-o", exe])
        yield exe


@pytest.fixture(scope="module")
def sampler():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sampler")
        subprocess.check_call(["g++", "-std=c++11", "-O2", os.path.join(ROOT, "examples", "example_sampler.cc")] + FLAGS + ["-o", exe])
        yield exe, d


@pytest.mark.gpu
@pytest.mark.parametrize("ladder", ["one", "many"])
def test_facade_gives_the_same_split_rhat_from_the_device_and_from_the_host_estimator(rhat_device, ladder):
    args = ["4000"] + (["many"] if ladder == "many" else [])
    dev, host = (run(rhat_device, args, host=h) for h in (False, True))
    print("\n".join(l for l in dev if not l.startswith("sequence")))
    counts = dev[0].split()
    assert counts[0] == "counts" and len(counts) == 6
    if ladder == "many":
        assert len(set(counts[1:])) >= 2                             # the replicas' windows on rung 1 are not the same rows
    queries = {w: [l for l in out if l.startswith("query")] for w, out in (("dev", dev), ("host", host))}
    assert len(queries["dev"]) == 4
    assert all(l.endswith("device=1") for l in queries["dev"]) and all(l.endswith("device=0") for l in queries["host"])
    strip = lambda out: [l.split(" device=")[0] for l in out]
    assert strip(dev) == strip(host)                                 # every %.17g value: features and sequences
    feats = [l.split() for l in dev if l.startswith("feature")]
    assert len(feats) == 3 + 2 + 3 + 1 and len([l for l in dev if l.startswith("sequence")]) == 10 * (3 + 2 + 3 + 1)
    assert all(0.7 < float(f[3]) < 10 for f in feats), feats


@pytest.mark.gpu
def test_host_side_proposals_use_the_host_estimator(rhat_device):
    out = run(rhat_device, ["2000", "hostprop"])
    queries = [l for l in out if l.startswith("query")]
    assert len(queries) == 4 and all(l.endswith("device=0") for l in queries)
    feats = [l.split() for l in out if l.startswith("feature")]
    assert len(feats) == 9 and all(0.7 < float(f[3]) < 10 for f in feats), feats


@pytest.mark.gpu
def test_sampler_prints_split_rhat_and_stops_on_it(sampler):
    exe, d = sampler
    common = ["--pt=8", "--replicas=3", "--nevery=500"]
    # a bound nothing misses: the run ends at the first test that has at least 4 rows
    out = run(exe, [os.path.join(d, "stop")] + common + ["--chain_rhat_stop=1e9"])
    lines = [RHAT_LINE.match(l) for l in out if l.startswith("Split R-hat")]
    assert len(lines) == 1 and lines[0], [l for l in out if "R-hat" in l]
    nrep, nrows, mx, par = lines[0].groups()
    assert int(nrep) == 3 and int(nrows) >= 4 and int(nrows) % 2 == 0 and 0.7 < float(mx) < 1e9 and 0 <= int(par) < 3
    assert any("Stopping based on chain_rhat_stop criterion." in l for l in out)
    steps = [int(l.split("step")[1]) for l in out if l.startswith("chain 0 step")]
    assert steps[-1] == 2000, steps                                  # tests at steps 0 (no rows yet) and 2000
    # the host estimator prints the same line
    assert [l for l in run(exe, [os.path.join(d, "stoph")] + common + ["--chain_rhat_stop=1e9"], host=True) if l.startswith("Split R-hat")] == [lines[0].group(0)]
    # a bound nothing meets (rhat^2 >= (n - 1) / n >= 1 / 2, and a NaN is below nothing): the run goes to its end
    out = run(exe, [os.path.join(d, "never")] + common + ["--nsteps=8000", "--chain_rhat_stop=0.5"])
    lines = [RHAT_LINE.match(l) for l in out if l.startswith("Split R-hat")]
    assert len(lines) == 4 and all(lines), [l for l in out if "R-hat" in l]
    assert not any("chain_rhat_stop" in l for l in out)
    assert [int(l.split("step")[1]) for l in out if l.startswith("chain 0 step")][-1] == 8000
    assert [int(m.group(2)) for m in lines] == sorted(int(m.group(2)) for m in lines) and int(lines[-1].group(2)) > int(lines[0].group(2))
    # the flag unset: no R-hat line
    out = run(exe, [os.path.join(d, "unset")] + common)
    assert not any("R-hat" in l for l in out)
