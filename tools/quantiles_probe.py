#!/usr/bin/env python3
"""quantiles_probe.py -- times the exact posterior quantiles of the cold rung (ptm_quantiles, on the device's own history ring)
against the path a caller had before it: the read-back of the ring (ptm_get_history) plus np.partition on the host.  Shapes: 32
dimensions x 16384 replicas x 1000 saved rows and 6 x 64 x 10000, each with the path left to the library, forced to the ring and
forced to pack; and a three-valued feature (ties keep every key a candidate) beside a continuous one, as series of 16384 x 1000
values.  `repeats` timings each: median and spread.  Every step is a process of its own under its own time limit, and the first
one that fails ends the probe.  Writes profiles/quantiles_device.json.

  usage: quantiles_probe.py [--repeats N] [--steps large,small,ties] [--no-host] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "quantiles_device.json")
PROBS = [0.05, 0.5, 0.95]
STEPS = {   # name: (shape, time limit of the step in seconds)
    "large": (dict(dim=32, replicas=16384, rows=1000), 420),
    "small": (dict(dim=6, replicas=64, rows=10000), 120),
    "ties": (dict(dim=1, replicas=16384, rows=1000), 180),
}
PATHS = {"default": {}, "ring": {"PTM_QUANTILES_PATH": "ring"}, "packed": {"PTM_QUANTILES_PATH": "packed"}}


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def set_path(env):
    for name in ("PTM_QUANTILES_PATH", "PTM_QUANTILES_PACK_BYTES", "PTM_QUANTILES_TILE"):
        os.environ.pop(name, None)
    os.environ.update(env)


def probe_ring(shape, repeats, host_path):
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
    N = W * rows
    ring_bytes = 8.0 * N * D
    out = {"shape": dict(shape, n_rungs=nt, add_every_n=1, ring_rows=rows + 2, rung=0, nfeat=D, nrows=rows, probs=PROBS), "paths": {}, "ptm_calibrate": cal}
    answers = {}
    for name, env in PATHS.items():
        set_path(env)
        eng.posterior_quantiles(PROBS, 0, D, rows)                   # (the workspace is there from here on)
        clock, events = [], []
        for _ in range(repeats):
            eng.timer_start()
            t0 = time.perf_counter()
            got = eng.posterior_quantiles(PROBS, 0, D, rows, brackets=True)
            clock.append(1e3 * (time.perf_counter() - t0))
            events.append(eng.timer_stop())
        packed, ring_passes, packed_passes = E.quantiles_last_path()
        print("[quantiles_probe] %s: %s ms (events), packed %s, %d + %d passes" % (name, events, packed, ring_passes, packed_passes), flush=True)
        answers[name] = got
        # walks over the ring: the bits pre-pass, the ring's digit passes and, where the call packed, the copy
        walks = 1 + ring_passes + (1 if packed else 0)
        out["paths"][name] = {"call_host_clock": spread(clock), "call_stream_events": spread(events), "packed": packed, "ring_passes": ring_passes,
                              "packed_passes": packed_passes, "walks_over_the_ring": walks,
                              "bytes_of_a_walk": ring_bytes,
                              "achieved_TBs_per_walk (the whole call's time over its walks: an upper bound of a walk's time, no counters collected)":
                                  ring_bytes * walks / (statistics.median(events) * 1e-3) / 1e12}
    set_path({})
    out["paths_agree_bit_for_bit"] = all(all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(answers[n], answers["default"])) for n in answers)
    if host_path:
        read, host = [], []
        same = None
        ranks = sorted({int(np.floor((N - 1) * p)) for p in PROBS} | {min(int(np.floor((N - 1) * p)) + 1, N - 1) for p in PROBS})
        for _ in range(repeats):
            t0 = time.perf_counter()
            hist = eng.history()
            read.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            x = hist["x"][1:rows + 1, :W].reshape(N, D)               # rows 1 .. newest of every walker (the ring has not wrapped)
            part = np.partition(np.ascontiguousarray(x.T), ranks, axis=1)   # (a feature's sample contiguous: the fast way round)
            lo = np.stack([part[:, int(np.floor((N - 1) * p))] for p in PROBS])
            host.append(1e3 * (time.perf_counter() - t0))
            same = bool(lo.tobytes() == np.asarray(answers["default"][1]).tobytes())
            print("[quantiles_probe] host: read %.0f ms, partition %.0f ms, same %s" % (read[-1], host[-1], same), flush=True)
            del hist, x, part
        out["host_path"] = {"ptm_get_history": spread(read), "numpy_partition": spread(host), "order_statistics_equal_the_device's_bits": same,
                            "read_back_bytes": float((rows + 2) * W * (D * 8 + 8 * 3 + 16))}
        total = [r + h for r, h in zip(read, host)]
        out["host_path"]["total"] = spread(total)
        for name, p in out["paths"].items():
            p["ratio_host_path_over_call"] = statistics.median(total) / p["call_host_clock"]["median_ms"]
            p["outside_the_host_path's_spread_on_the_fast_side"] = p["call_host_clock"]["max_ms"] < min(total)
    eng.close()
    return out


def probe_ties(shape, repeats):
    """a three-valued feature beside a continuous one, as a caller's series: the call's time holds the upload of the series"""
    import numpy as np
    from ptmcmc_amd import engine as E
    W, rows = shape["replicas"], shape["rows"]
    N = W * rows
    rng = np.random.default_rng(5)
    series = {"three values": rng.permutation(np.repeat([-1.5, 2.0, 2.0000000000000004], [N // 3, N // 3, N - 2 * (N // 3)])).reshape(rows, W, 1),
              "continuous": rng.standard_normal((rows, W, 1))}
    out = {"shape": dict(shape, probs=PROBS, series_bytes=8.0 * N), "cases": {},
           "note": "ptm_quantiles_series: every timing holds the allocation and the upload of the series"}
    for what, x in series.items():
        for name, env in PATHS.items():
            set_path(env)
            E.quantiles_series(x, PROBS)
            clock = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                got = E.quantiles_series(x, PROBS, brackets=True)
                clock.append(1e3 * (time.perf_counter() - t0))
            packed, ring_passes, packed_passes = E.quantiles_last_path()
            s = np.sort(x.reshape(N))
            same = bool(all(got[1][k, 0] == s[int(np.floor((N - 1) * p))] for k, p in enumerate(PROBS)))
            out["cases"]["%s, %s" % (what, name)] = {"call_host_clock": spread(clock), "packed": packed, "ring_passes": ring_passes, "packed_passes": packed_passes,
                                                      "order_statistics_equal_np_sort": same}
    set_path({})
    return out


def run_step(args):
    shape, _ = STEPS[args.step]
    result = probe_ties(shape, args.repeats) if args.step == "ties" else probe_ring(shape, args.repeats, not args.no_host)
    with open(args.part, "w") as f:
        json.dump(result, f)


def run_probe(args):
    out = {"what": "exact posterior quantiles of the cold rung at population shapes (MI355X): ptm_quantiles on the device's own history ring against "
                   "ptm_get_history plus np.partition on the host (tools/quantiles_probe.py; a process per step, the repeats of a path in a row; "
                   "host clock around the calls and stream events; medians with the spread).  No hardware counters were collected: the bytes per "
                   "second of a walk are estimates from the call's time and the algorithm's bytes.",
           "steps": {}}
    with tempfile.TemporaryDirectory() as d:
        for step in args.steps.split(","):
            part = os.path.join(d, step + ".json")
            cmd = ["timeout", "-k", "10", str(STEPS[step][1]), sys.executable, os.path.abspath(__file__), "--step", step, "--part", part, "--repeats", str(args.repeats)]
            if args.no_host:
                cmd.append("--no-host")
            print("[quantiles_probe]", " ".join(cmd), flush=True)
            rc = subprocess.call(cmd)
            if rc:
                print("[quantiles_probe] step %s ended with status %d: nothing more is started" % (step, rc), flush=True)
                out["steps"][step] = {"failed_with_status": rc}
                break
            with open(part) as f:
                out["steps"][step] = json.load(f)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))
    return 1 if any("failed_with_status" in v for v in out["steps"].values()) else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", default="large,small,ties")
    ap.add_argument("--no-host", action="store_true", help="time the device call alone")
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--step", help="(internal) run one step in this process")
    ap.add_argument("--part", help="(internal) where the step writes its result")
    a = ap.parse_args()
    if a.step:
        run_step(a)
    else:
        sys.exit(run_probe(a))
