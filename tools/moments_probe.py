#!/usr/bin/env python3
"""moments_probe.py -- times the pooled posterior moments of the cold rung (ptm_moments, on the device's own history ring) against
the path a caller had before it: the read-back of the ring (ptm_get_history) plus a host pass over it.  Two shapes, 32 dimensions x
16384 replicas x 1000 saved rows and 6 x 64 x 1000, in one process, the two paths alternating; medians and the spread of `repeats`
timings.  The host pass is numpy's (the mean, then one matrix product of the centred rows): faster than the facade's sequential
moments_estimator, so the comparison flatters the host.  Writes profiles/moments_device.json.

  usage: moments_probe.py [--repeats N] [--small-only | --large-only] [--no-host] [--out FILE]
         moments_probe.py --merge-stats KERNEL_STATS_CSV [--out FILE]    add to FILE the per-kernel times, with achieved bytes/s, of a
                                                                         second run, `--large-only --no-host --out OTHER`, under
                                                                         rocprofv3 --kernel-trace --stats --output-format csv
         moments_probe.py --record FILE     run examples/example_sampler.cc (default recipe, 3 replicas) without a covariance flag
                                            and store its proposal lines and chain files in FILE (tests/golden/sampler_chain_files.json.gz)
"""
import argparse
import csv
import gzip
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "moments_device.json")
SHAPES = [dict(dim=32, replicas=16384, rows=1000), dict(dim=6, replicas=64, rows=1000)]
# the recorded sampler run (tests/test_gpu_moments_facade.py repeats it)
RECORD_ARGS = ["--default_recipe", "--replicas=3", "--nsteps=1000", "--nevery=500"]


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def probe_shape(shape, repeats, host_path=True):
    import numpy as np
    from ptmcmc_amd import engine as E
    from ptmcmc_amd.problems import GaussianProblem
    D, W, rows = shape["dim"], shape["replicas"], shape["rows"]
    nt = 2
    pr = GaussianProblem(D, nt, 1e2)
    eng = E.Engine(D, nt, W, seed=0x5EED0A01, swap_rate=0.1, add_every_n=1, history_rungs=1, history_capacity=rows + 2)
    pr.configure(eng, E.PROP_LOWER)
    eng.init_from_prior()
    eng.step(rows)
    eng.sync()
    cal = eng.calibrate()
    eng.posterior_moments(0, D, rows)                                # (the workspace is there from here on)
    dev, dev_events, read, host = [], [], [], []
    same = None
    for _ in range(repeats):
        eng.timer_start()
        t0 = time.perf_counter()
        mean, cov, var, n = eng.posterior_moments(0, D, rows)
        dev.append(1e3 * (time.perf_counter() - t0))
        dev_events.append(eng.timer_stop())
        if not host_path:
            continue
        t0 = time.perf_counter()
        hist = eng.history()
        read.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        newest = 1 + (eng.nhist.reshape(nt, W)[0].astype(np.int64) - 1)
        assert (newest == rows).all()
        x = hist["x"][1:rows + 1, :W].reshape(rows * W, D)          # rows 1 .. newest of every walker (the ring has not wrapped)
        m = x.mean(axis=0)
        d = x - m
        c = d.T @ d / (rows * W - 1)
        host.append(1e3 * (time.perf_counter() - t0))
        same = bool(np.allclose(c, cov, rtol=1e-9, atol=1e-12) and np.allclose(m, mean, rtol=1e-12, atol=1e-12))
        del hist, x, d
    eng.close()
    P = D * (D + 1) // 2
    per_lane = min(4, (P + 255) // 256)                             # (the cross kernel's pairs a lane, and its chunks of pairs a walker)
    chunks = (P + 256 * per_lane - 1) // (256 * per_lane)
    if not host_path:
        read, host = [float("nan")], [float("nan")]
    return {
        "shape": dict(shape, n_rungs=nt, add_every_n=1, ring_rows=rows + 2, rung=0, nfeat=D, nrows=rows, pairs=P),
        "ptm_moments_call_host_clock": spread(dev),
        "ptm_moments_call_stream_events": spread(dev_events),
        "host_path": {"ptm_get_history": spread(read), "numpy_mean_and_matrix_product": spread(host), "agrees_with_device_to_1e-9": same,
                      "read_back_bytes": float((rows + 2) * W * (D * 8 + 8 * 3 + 16))},
        "ratio_host_path_over_call": (statistics.median(read) + statistics.median(host)) / statistics.median(dev),
        "ptm_calibrate": cal,
        "algorithmic_bytes": {"moments_sum_kernel": 8.0 * rows * W * D, "moments_cross_kernel": 8.0 * rows * W * D * chunks + 8.0 * W * P,
                              "moments_block_kernel (pairs)": 8.0 * W * P},
    }


def run_probe(args):
    out = {"what": "pooled posterior moments of the cold rung at population shapes (MI355X): ptm_moments on the device's own history ring against "
                   "ptm_get_history plus a numpy pass on the host (tools/moments_probe.py; one process, the paths alternating; host clock "
                   "around the calls; medians with the spread)",
           "shapes": [probe_shape(s, args.repeats, not args.no_host) for s in (SHAPES[1:] if args.small_only else SHAPES[:1] if args.large_only else SHAPES)]}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


def merge_stats(args):
    """per-kernel averages of a rocprofv3 --kernel-trace --stats run of this probe at the large shape alone"""
    with open(args.out) as f:
        out = json.load(f)
    kernels = {}
    with open(args.merge_stats) as f:
        for row in csv.DictReader(f):
            if "moments_" in row["Name"]:
                kernels[row["Name"].split("(")[0].replace("void ptm::", "")] = {
                    "calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    out["kernels_of_the_large_shape_under_rocprofv3_kernel_trace (a second run; every call of it)"] = kernels
    big = out["shapes"][0]
    for name, k in kernels.items():
        for key, nbytes in big["algorithmic_bytes"].items():
            if key.split(" ")[0] in name and "(pairs)" not in key:
                k["algorithmic_bytes"] = nbytes
                k["achieved_TBs"] = nbytes / (k["avg_us"] * 1e-6) / 1e12
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(kernels, indent=1))


def sampler_record(exe_dir=None, extra=()):
    """the recorded run: {"proposal": the lines from "Proposal distribution is:" up to the run's first line, "files": {name: text}}"""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(exe_dir or d, "example_sampler_fx")
        if not os.path.exists(exe):
            subprocess.check_call(["g++", "-std=c++11", "-O2", os.path.join(ROOT, "examples", "example_sampler.cc"), "-I", os.path.join(ROOT, "include"), "-I",
                                   os.path.join(ROOT, "ptmcmc_amd", "host"), "-L", os.path.join(ROOT, "ptmcmc_amd"), "-lptm_engine",
                                   "-Wl,-rpath," + os.path.join(ROOT, "ptmcmc_amd"), "-pthread", "-o", exe])
        run = os.path.join(d, "run")
        os.makedirs(run)
        r = subprocess.run([exe, os.path.join(run, "chain")] + RECORD_ARGS + list(extra), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = r.stdout.splitlines()
        a = lines.index("Proposal distribution is:")
        b = next(i for i in range(a, len(lines)) if lines[i].startswith("Running chain") or lines[i].startswith("ptmcmc_sampler::initialize"))
        return {"args": RECORD_ARGS, "proposal": [l for l in lines[a:b] if l.strip()], "files": {n: open(os.path.join(run, n)).read() for n in sorted(os.listdir(run))},
                "stdout": lines}


def record(args):
    rec = sampler_record(exe_dir=args.exe_dir)
    del rec["stdout"]
    with gzip.GzipFile(args.record, "wb", mtime=0) as f:
        f.write(json.dumps(rec, indent=0, sort_keys=True).encode())
    print("recorded %d files, %d bytes of text, %d proposal lines -> %s" % (len(rec["files"]), sum(len(v) for v in rec["files"].values()), len(rec["proposal"]), args.record))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--large-only", action="store_true")
    ap.add_argument("--no-host", action="store_true", help="time the device call alone")
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--merge-stats")
    ap.add_argument("--record")
    ap.add_argument("--exe-dir", help="--record: a directory that already holds example_sampler_fx (a build against another commit's library)")
    a = ap.parse_args()
    if a.record:
        record(a)
    elif a.merge_stats:
        merge_stats(a)
    else:
        run_probe(a)
