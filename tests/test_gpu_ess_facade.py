"""The facade's effective-sample-size report on the device (tests/cxx/ess_device_main.cc): report_effective_samples estimates from the
device's own ring -- the same %.17g values as the host estimator (PTM_HOST_ESS=1), the device path taken only without it -- and
report_effective_samples_all gives every replica the answer of the host estimator on that replica's rows."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_sampler(out):
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ptmcmc_amd", "host"),
                           os.path.join(ROOT, "examples", "example_sampler.cc"), "-L", os.path.join(ROOT, "ptmcmc_amd"), "-lptm_engine",
                           "-Wl,-rpath," + os.path.join(ROOT, "ptmcmc_amd"), "-pthread", "-o", out])


@pytest.mark.gpu
def test_sampler_population_prints_its_spread_and_stops_where_replica_0_says():
    """--replicas=3 --chain_ess_stop on an 8-rung ladder: after replica 0's line (the reference's, and the stop criterion) one line
    with the population's min / median / max, all from one device estimate; the host path (PTM_HOST_ESS=1) prints the same
    replica-0 lines and stops at the same step."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sampler")
        build_sampler(exe)
        runs = {}
        for where in ("device", "host"):
            env = dict(os.environ)
            env.pop("PTM_HOST_ESS", None)
            if where == "host":
                env["PTM_HOST_ESS"] = "1"
            r = subprocess.run([exe, os.path.join(d, where), "--pt=8", "--replicas=3", "--nsteps=40000", "--nevery=500", "--chain_ess_stop=25"],
                               capture_output=True, text=True, timeout=600, env=env)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            runs[where] = r.stdout.splitlines()
        dev, host = runs["device"], runs["host"]
        cold = [i for i, l in enumerate(dev) if l.startswith("Over 3 pars: ess=")]
        assert cold
        for i in cold:
            assert dev[i + 1].startswith("Over 3 replicas: ess min="), dev[i:i + 2]
            lo, mid, hi = (float(dev[i + 1].split(k + "=")[1].split()[0]) for k in ("min", "median", "max"))
            own = float(dev[i].split("ess=")[1].split()[0])
            assert lo <= mid <= hi and lo <= own <= hi, dev[i:i + 2]
        assert not [l for l in host if "replicas: ess min" in l]
        assert [dev[i] for i in cold] == [l for l in host if l.startswith("Over 3 pars: ess=")]
        steps = {w: [int(l.split("step")[1]) for l in runs[w] if l.startswith("chain 0 step")] for w in runs}
        assert steps["device"] == steps["host"] and steps["device"][-1] < 40000
        assert any("Stopping based on chain_ess_stop" in l for l in dev) and any("Stopping based on chain_ess_stop" in l for l in host)


@pytest.mark.gpu
@pytest.mark.parametrize("ladder", ["one", "many"])
def test_facade_reports_the_same_effective_sample_size_from_the_device_and_for_every_replica(ladder):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "essdev")
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ptmcmc_amd", "host"),
                               os.path.join(ROOT, "tests", "cxx", "ess_device_main.cc"), "-L", os.path.join(ROOT, "ptmcmc_amd"), "-lptm_engine",
                               "-Wl,-rpath," + os.path.join(ROOT, "ptmcmc_amd"), "-pthread", "-o", exe])
        outs = {}
        for where in ("device", "host"):
            env = dict(os.environ)
            env.pop("PTM_HOST_ESS", None)
            if where == "host":
                env["PTM_HOST_ESS"] = "1"
            r = subprocess.run([exe, "4000"] + (["many"] if ladder == "many" else []), capture_output=True, text=True, timeout=300, env=env)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            outs[where] = [ln.split() for ln in r.stdout.strip().splitlines()]
            print(where, r.stdout)
        # (also with five exchange candidates per step the cold chains agree on their add_state counts: the coldest rung has one
        #  neighbour and is never exchanged twice in a step -- the device path is the one taken on long ladders too)
        counts = set(outs["device"][0][1:])
        assert outs["device"][0][0] == "counts" and counts == {"4000"}, outs["device"][0]
        cold = {w: [ln for ln in outs[w] if ln[0] == "cold"] for w in outs}
        assert len(cold["device"]) == 3
        for dev, host in zip(cold["device"], cold["host"]):
            assert dev[:4] == host[:4], (dev, host)                      # query, ess (%.17g), length
            assert dev[4] == "device=1" and host[4] == "device=0"
        assert any(float(ln[2]) > 0 for ln in cold["device"])
        reps = [ln for ln in outs["device"] if ln[0] == "replica"]
        assert len(reps) == 3 * 5
        for ln in reps:
            assert ln[3:5] == ln[6:8], ln                                # the population entry point == the host estimator on that replica's rows
            if ln[2] == "0":
                assert ln[3:5] == cold["device"][int(ln[1])][2:4], ln    # entry 0 is the cold chain's answer
        assert len({ln[3] for ln in reps if ln[1] == "0"}) == 5          # five replicas, five different chains
        assert [ln for ln in outs["host"] if ln[0] == "replica"] == reps
