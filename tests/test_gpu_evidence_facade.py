"""The facade's log-evidence (parallel_tempering_chains with do_evid, the sampler's --pt_stop_evid_err): the device path and the host
path (PTM_HOST_EVIDENCE=1) print the same %.17g totals, records and best standard error at every statistics bin, the chains are
those of a run without it, the sampler stops where the criterion says, and a checkpointed run continues the uninterrupted one."""
import os
import subprocess
import tempfile
import time

import pytest

from test_gpu_ess_facade import ROOT, build_sampler

EVID_LINES = ("Total log-evidence:", "total_evidence_records[", "total_log_evs:", "recent ev analysis:", "i=")


def run(cmd, host, cwd=None, timeout=900):
    env = dict(os.environ)
    env.pop("PTM_HOST_EVIDENCE", None)
    if host:
        env["PTM_HOST_EVIDENCE"] = "1"
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=cwd)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def evid_exe():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "eviddev")
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ptmcmc_amd", "host"),
                               os.path.join(ROOT, "tests", "cxx", "evidence_device_main.cc"), "-L", os.path.join(ROOT, "ptmcmc_amd"), "-lptm_engine",
                               "-Wl,-rpath," + os.path.join(ROOT, "ptmcmc_amd"), "-pthread", "-o", exe])
        yield exe


@pytest.mark.gpu
@pytest.mark.parametrize("replicas", [1, 3])
def test_device_and_host_paths_agree_at_every_bin_and_the_chains_are_untouched(evid_exe, replicas):
    dev = run([evid_exe, "3500", str(replicas)], host=False)
    host = run([evid_exe, "3500", str(replicas)], host=True)
    plain = run([evid_exe, "3500", str(replicas), "noevid"], host=False)
    assert dev == host
    bins = [l.split() for l in dev if l.startswith("bin ")]
    assert len(bins) == 7 * replicas and [b[1] for b in bins[::replicas]] == [str(k) for k in range(1, 8)]
    for b in bins:
        assert (float(b[6]) < 1e100) == (int(b[1]) >= 6), b          # the first standard error after six bins
    assert len([l for l in dev if l.startswith("Total log-evidence:")]) == 7          # replica 0's lines only
    spread = [l for l in dev if l.startswith("Over %d replicas: log-evidence min=" % replicas)]
    assert len(spread) == (7 if replicas > 1 else 0)
    for l in spread:
        lo, mid, hi = (float(l.split(k + "=")[1].split()[0]) for k in ("min", "median", "max"))
        assert lo <= mid <= hi
    if replicas > 1:
        assert len({b[4] for b in bins if b[1] == "7"}) == replicas          # three replicas, three different ladders
    assert any(l.startswith("Best evidence stderr=") for l in dev) and any(l.startswith(" log eratio:(") for l in dev)
    states = [l for l in dev if l.startswith("state ")]
    assert len(states) == 4 * replicas and states == [l for l in plain if l.startswith("state ")]
    assert not [l for l in plain if l.startswith(EVID_LINES) or l.startswith("Best evidence")]


def evidence_lines(lines):
    """what the statistics block prints: from "Total log-evidence:" to the last line of its "recent ev analysis" """
    out, inside = [], False
    for l in lines:
        if l.startswith("Total log-evidence:"):
            inside = True
        elif inside and not (l.startswith(EVID_LINES) or "\t" in l or (l[:1].isdigit() and ": N=" in l)):
            inside = False
        if inside:
            out.append(l)
    return out


@pytest.mark.gpu
def test_sampler_stops_on_pt_stop_evid_err_and_a_restart_continues_the_run():
    """--pt=8 --save_every=1: bins of 10000 steps, the first standard error after six of them.  A huge bound stops at the report of
    step 60000; a bound of 1e-300 never does; the host path prints the same lines; a run checkpointed between two bins and
    restarted prints the evidence lines of the uninterrupted run."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sampler")
        build_sampler(exe)
        common = ["--pt=8", "--nevery=500", "--save_every=1", "--nsteps=62000"]
        t0 = time.time()
        dev = run([exe, os.path.join(d, "dev")] + common + ["--pt_stop_evid_err=1e99"], host=False)
        t_dev = time.time() - t0
        host = run([exe, os.path.join(d, "host")] + common + ["--pt_stop_evid_err=1e99"], host=True)
        t_host = time.time() - t0 - t_dev
        steps = [int(l.split("step")[1]) for l in dev if l.startswith("chain 0 step")]
        assert steps[-1] == 60000 and any("Stopping based on pt_stop_evid_err criterion." in l for l in dev)
        assert len([l for l in dev if l.startswith("Total log-evidence:")]) == 6
        assert evidence_lines(dev) == evidence_lines(host) and len(evidence_lines(dev)) > 20
        assert steps == [int(l.split("step")[1]) for l in host if l.startswith("chain 0 step")]
        never = run([exe, os.path.join(d, "never")] + common + ["--pt_stop_evid_err=1e-300"], host=False)
        assert [int(l.split("step")[1]) for l in never if l.startswith("chain 0 step")][-1] == 62000
        assert not any("Stopping based on pt_stop_evid_err" in l for l in never)
        assert evidence_lines(never) == evidence_lines(dev)
        first = run([exe, "cp"] + common + ["--pt_stop_evid_err=1e99", "--checkp_at_step=25300"], host=False, cwd=d)
        assert os.path.exists(os.path.join(d, "step_25300-cp", "chain0-cp", "PTevidence.cp"))
        second = run([exe, "cp"] + common + ["--pt_stop_evid_err=1e99", "--restart_dir=" + os.path.join(d, "step_25300-cp")], host=False, cwd=d)
        assert len(evidence_lines(first)) > 0 and evidence_lines(first) + evidence_lines(second) == evidence_lines(dev)
        assert any("Stopping based on pt_stop_evid_err criterion." in l for l in second)
        print("sampler, 60000 steps of an 8-rung ladder with six evidence bins: device path %.1f s, host path %.1f s" % (t_dev, t_host))
