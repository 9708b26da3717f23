"""The facade's corner-plot histograms (tests/cxx/histograms_device_main.cc): parallel_tempering_chains::posterior_histograms counts
on the device's own ring -- the same integers as the host estimator (PTM_HOST_HISTOGRAMS=1), the device path taken only without it.
The sampler's --corner_out writes the cold rung's counts to a file and says so in one line (tests/cxx/histograms_sampler_main.cc);
the file reads back with read_corner, its 1-D counts are np.histogram's of the read-back cold chains over the same window and
ranges, and the host estimator writes the same file."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import histograms_model as H
from ptmcmc_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ptmcmc_amd", "host"), "-L", os.path.join(ROOT, "ptmcmc_amd"), "-lptm_engine",
         "-Wl,-rpath," + os.path.join(ROOT, "ptmcmc_amd"), "-pthread"]
CORNER_LINE = re.compile(r"^Posterior histograms over (\d+) replicas, (\d+) rows: (\d+) parameters, (\d+) pairs, (\d+) bins \((device|host)\), written to (\S+)$")

pytestmark = pytest.mark.gpu


def run(exe, args, host=False, timeout=300, expect=0):
    env = dict(os.environ)
    env.pop("PTM_HOST_HISTOGRAMS", None)
    if host:
        env["PTM_HOST_HISTOGRAMS"] = "1"
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == expect, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def build(d, name, source):
    exe = os.path.join(d, name)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "cxx", source)] + FLAGS + ["-o", exe])
    return exe


@pytest.fixture(scope="module")
def histograms_device():
    with tempfile.TemporaryDirectory() as d:
        yield build(d, "histogramsdev", "histograms_device_main.cc")


@pytest.fixture(scope="module")
def sampler():
    with tempfile.TemporaryDirectory() as d:
        yield build(d, "histogramssampler", "histograms_sampler_main.cc"), d


def ints(out, tag, q):
    return np.array([[int(v) for v in l.split()[2:]] for l in out if l.startswith("%s %d " % (tag, q))], dtype=np.int64)


def near_a_twentieth(outside, n):
    """the samples outside a range that ends at the 5% and 95% points of the sample itself: with h = 0.05 (n - 1) (or 0.95 (n - 1))
    and no ties, floor(h) + 1 or n - 1 - floor(h) of them, within 1 of n / 20; a chain that rejected its proposals repeats its state,
    and the values equal to an end lie inside -- fewer outside by the length of such a run (50 saved rows and more: 100 rejections in
    a row, never at these acceptance rates)"""
    return bool((outside <= 0.05 * n + 1).all() and (outside >= 0.05 * n - 50).all())


@pytest.mark.parametrize("ladder", ["one", "many"])
def test_facade_gives_the_same_counts_from_the_device_and_from_the_host_estimator(histograms_device, ladder):
    args = ["2000"] + (["many"] if ladder == "many" else [])
    dev, host = (run(histograms_device, args, host=h) for h in (False, True))
    counts = dev[0].split()
    assert counts[0] == "counts" and len(counts) == 71
    if ladder == "many":
        assert len(set(counts[1:])) >= 2                             # the replicas' windows on rung 1 are not the same rows
    queries = {w: [l for l in out if l.startswith("query")] for w, out in (("dev", dev), ("host", host))}
    assert len(queries["dev"]) == 5
    assert all(l.endswith("device=1") for l in queries["dev"]) and all(l.endswith("device=0") for l in queries["host"])
    got = [int(l.split()[7].split("=")[1]) for l in queries["dev"]]
    assert got[:2] == [35000, 17500] and got[3] == 70 and got[4] == 21000 and (got[2] == 70000 if ladder == "one" else got[2] >= 70000)
    strip = lambda out: [l.split(" device=")[0] for l in out]
    assert strip(dev) == strip(host)                                 # every integer, and the ranges
    # what the counts owe each other
    for q, (nf, nbins, n, pairs, whole) in enumerate(((3, 20, got[0], 3, True), (2, 7, got[1], 1, False), (3, 128, got[2], 3, False), (1, 1, 70, 0, True), (3, 20, 21000, 0, False))):
        h1, h2, below, above = ints(dev, "h1", q), ints(dev, "h2", q), ints(dev, "below", q)[0], ints(dev, "above", q)[0]
        assert h1.shape == (nf, nbins) and h2.shape[0] == pairs and np.array_equal(below + above + h1.sum(axis=1), np.full(nf, n))
        if whole:
            assert (below == 0).all() and (above == 0).all() and (h1[:, 0] >= 1).all() and (h1[:, -1] >= 1).all()   # the minimum and the maximum
        else:
            assert near_a_twentieth(below, n) and near_a_twentieth(above, n)                                      # the 5% and 95% points
        for p, (i, j) in enumerate(H.pairs(nf) if pairs else []):
            t = h2[p].reshape(nbins, nbins)
            assert (t.sum(axis=1) <= h1[i]).all() and (t.sum(axis=0) <= h1[j]).all() and t.sum() >= n - below[i] - above[i] - below[j] - above[j]


def test_host_side_proposals_use_the_host_estimator(histograms_device):
    out = run(histograms_device, ["1000", "hostprop"])
    queries = [l for l in out if l.startswith("query")]
    assert len(queries) == 5 and all(l.endswith("device=0") for l in queries)
    h1 = ints(out, "h1", 0)
    assert h1.shape == (3, 20) and (h1.sum(axis=1) == 35000).all()


def test_sampler_writes_the_corner_file_and_its_counts_are_numpys(sampler):
    exe, d = sampler
    common = ["--replicas=70", "--nsteps=1000", "--nevery=500"]
    path = os.path.join(d, "posterior.corner")
    out = run(exe, [os.path.join(d, "first")] + common + ["--corner_out=" + path])
    lines = [CORNER_LINE.match(l) for l in out if l.startswith("Posterior histograms")]
    assert len(lines) == 1 and lines[0], [l for l in out if "histograms" in l]
    nrep, nrows, npar, npairs, nbins, where, written = lines[0].groups()
    assert (int(nrep), int(npar), int(npairs), int(nbins), where, written) == (70, 3, 3, 20, "device", path) and int(nrows) >= 100
    c = E.read_corner(path)
    N = 70 * int(nrows)
    assert (c["dim"], c["nbins"], c["count"], c["replicas"], c["rows"], c["names"]) == (3, 20, N, 70, int(nrows), ["a", "b", "c"])
    assert c["pairs"] == [("a", "b"), ("a", "c"), ("b", "c")] and c["h2"].shape == (3, 20, 20)
    # the file's counts are the engine's own answer for the same rung, window, ranges and bins
    eng = [l.split() for l in out if l.startswith("engine")]
    assert eng[0] == ["engine", str(N), nrows, "20"]
    assert c["lo"].tobytes() == np.array([float(v) for v in eng[1][1:]]).tobytes() and c["hi"].tobytes() == np.array([float(v) for v in eng[2][1:]]).tobytes()
    assert np.array_equal(c["h1"], np.array([[int(v) for v in l[1:]] for l in eng[3:6]], dtype=np.int64))
    # ... and numpy's of the read-back cold chains: the range is the sample's minimum and maximum, so nothing lies outside
    cold = np.array([[float(v) for v in l.split()[2:]] for l in out if l.startswith("cold ")])
    assert cold.shape == (N, 3)
    assert c["lo"].tobytes() == cold.min(axis=0).tobytes() and c["hi"].tobytes() == cold.max(axis=0).tobytes()
    assert (c["below"] == 0).all() and (c["above"] == 0).all()
    for f in range(3):
        assert np.array_equal(c["h1"][f], np.histogram(cold[:, f], 20, (c["lo"][f], c["hi"][f]))[0]), f
    for p, (i, j) in enumerate(H.pairs(3)):
        want = np.histogram2d(cold[:, i], cold[:, j], 20, [(c["lo"][i], c["hi"][i]), (c["lo"][j], c["hi"][j])])[0]
        assert np.array_equal(c["h2"][p], want.astype(np.int64)), (i, j)
    # the host estimator writes the same file
    path_h = os.path.join(d, "posterior_host.corner")
    out_h = run(exe, [os.path.join(d, "firsth")] + common + ["--corner_out=" + path_h], host=True)
    assert [CORNER_LINE.match(l).group(6) for l in out_h if l.startswith("Posterior histograms")] == ["host"]
    assert open(path_h).read() == open(path).read()
    # other bins and a central share of the samples, at another ladder and population; bad flags are refused before anything runs
    path2 = os.path.join(d, "other.corner")
    out2 = run(exe, [os.path.join(d, "second"), "--replicas=33", "--pt=3", "--nsteps=400", "--nevery=200", "--corner_out=" + path2, "--corner_bins=7", "--corner_range=0.9"])
    m = [CORNER_LINE.match(l) for l in out2 if l.startswith("Posterior histograms")]
    assert len(m) == 1 and m[0].group(1, 5, 6) == ("33", "7", "device")
    c2 = E.read_corner(path2)
    n2 = c2["count"]
    assert c2["nbins"] == 7 and c2["h2"].shape == (3, 7, 7) and n2 == 33 * c2["rows"]
    assert near_a_twentieth(c2["below"], n2) and near_a_twentieth(c2["above"], n2)
    assert np.array_equal(c2["below"] + c2["above"] + c2["h1"].sum(axis=1), np.full(3, n2))
    cold2 = np.array([[float(v) for v in l.split()[2:]] for l in out2 if l.startswith("cold ")])
    for f in range(3):
        assert np.array_equal(c2["h1"][f], np.histogram(cold2[:, f], 7, (c2["lo"][f], c2["hi"][f]))[0]), f
    for flag in ("--corner_bins=0", "--corner_bins=129", "--corner_bins=x", "--corner_range=0", "--corner_range=1.5"):
        out3 = run(exe, [os.path.join(d, "third"), "--replicas=70", "--nsteps=400", "--corner_out=" + path2, flag], expect=1)
        assert any(flag.split("=")[0] in l for l in out3) and not any(l.startswith("chain 0 step") for l in out3), flag


def test_without_the_flag_nothing_is_said_or_written(sampler):
    exe, d = sampler
    out = run(exe, [os.path.join(d, "plain"), "--replicas=8", "--nsteps=200", "--nevery=100"])
    assert not any("histogram" in l.lower() for l in out) and not any(f.endswith(".corner") for f in os.listdir(d) if f.startswith("plain"))
