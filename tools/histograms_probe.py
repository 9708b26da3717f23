#!/usr/bin/env python3
"""histograms_probe.py -- times the corner-plot histograms of the cold rung (ptm_histograms, on the device's own history ring): the
1-D histograms alone, and with all pairs at 20 and at 64 bins; the two lane mappings of the 2-D kernel and tiles of pairs around the
default, at 20 bins.  Against two baselines: the path a caller had before -- the read-back of the cold chains
(ptm_get_history_chains) plus np.histogram / np.histogram2d on the host -- and a call of ptm_quantiles on the same ring over its
walks of the ring (the bits pre-pass and the digit passes: each a quantiles walk, the floor a ring walk can reach).  Shapes: 32
dimensions x 16384 replicas x 1000 saved rows and 6 x 64 x 10000.  `repeats` timings each, in a row: median and spread.

np.histogram2d over 16 M rows takes seconds a pair, and the large shape has 496 pairs: there the host path bins `--host-pairs` of
them, each timed, and is reported twice -- what was measured (the read-back, every 1-D histogram and those pairs: a lower bound of
the host path) and that with the pairs' mean time extrapolated to all pairs (named so).  The device call stays the default only if
its slowest repeat beats the measured lower bound's fastest.

Every step is a process of its own under its own time limit, and the first one that fails ends the probe.  Writes
profiles/histograms_device.json.

  usage: histograms_probe.py [--repeats N] [--steps large,small] [--no-host] [--host-pairs K] [--out FILE]
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
DEFAULT_OUT = os.path.join(ROOT, "profiles", "histograms_device.json")
STEPS = {   # name: (shape, time limit of the step in seconds)
    "large": (dict(dim=32, replicas=16384, rows=1000), 900),
    "small": (dict(dim=6, replicas=64, rows=10000), 240),
}
ENV = ("PTM_HIST_TILE", "PTM_HIST_MAP")


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def set_env(env):
    for name in ENV:
        os.environ.pop(name, None)
    os.environ.update(env)


def probe_ring(shape, repeats, host_path, host_pairs):
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
    N, npairs = W * rows, D * (D - 1) // 2
    ring_bytes = 8.0 * N * D
    ends, _ = eng.posterior_quantiles([0.0, 1.0], 0, D, rows)        # corner's default range: the minimum and the maximum
    lo, hi = ends[0].copy(), ends[1].copy()
    out = {"shape": dict(shape, n_rungs=nt, add_every_n=1, ring_rows=rows + 2, rung=0, nfeat=D, nrows=rows, npairs=npairs, ring_bytes=ring_bytes), "device": {}}

    def timed(call):
        call()                                                       # (the workspace and the code objects are there from here on)
        clock, events = [], []
        for _ in range(repeats):
            eng.timer_start()
            t0 = time.perf_counter()
            got = call()
            clock.append(1e3 * (time.perf_counter() - t0))
            events.append(eng.timer_stop())
        return got, {"call_host_clock": spread(clock), "call_stream_events": spread(events)}

    # the floor: a quantiles call's walks over the same ring
    set_env({})
    _, t = timed(lambda: eng.posterior_quantiles([0.5], 0, D, rows))
    _, ring_passes, _ = E.quantiles_last_path()
    walks = 1 + ring_passes
    t.update({"walks_over_the_ring": walks, "ms_per_walk (the call's time over its walks: an upper bound of one quantiles walk, no counters collected)":
              t["call_stream_events"]["median_ms"] / walks})
    out["quantiles_walk"] = t
    floor = t["call_stream_events"]["median_ms"] / walks

    tile20 = max(1, min(npairs, 128 * 1024 // (4 * 20 * 20)))
    cases = [("1-D only, 20 bins", 20, False, {}), ("all pairs, 20 bins", 20, True, {}), ("all pairs, 64 bins", 64, True, {}), ("1-D only, 64 bins", 64, False, {}),
             ("all pairs, 20 bins, lanes over rows", 20, True, {"PTM_HIST_MAP": "rows"}), ("all pairs, 64 bins, lanes over rows", 64, True, {"PTM_HIST_MAP": "rows"})]
    for tp in sorted({max(1, tile20 // 4), max(1, tile20 // 2), max(1, 3 * tile20 // 4)}):
        if tp < tile20:
            cases.append(("all pairs, 20 bins, tile of %d pairs" % tp, 20, True, {"PTM_HIST_TILE": str(tp)}))
    answers = {}
    for name, nbins, pairs, env in cases:
        set_env(env)
        got, t = timed(lambda: eng.posterior_histograms(lo, hi, nbins, 0, D, rows, pairs=pairs))
        tiles, tp, mapping = E.histograms_last_launch()
        t.update({"nbins": nbins, "pairs": pairs, "tiles": tiles, "pairs_of_a_tile": tp, "mapping": mapping if pairs else None,
                  "over_one_quantiles_walk": t["call_stream_events"]["median_ms"] / floor})
        print("[histograms_probe] %s: %s" % (name, t), flush=True)
        key = (nbins, pairs)
        if key in answers:
            t["same_counts_as_the_default"] = bool(all(np.array_equal(a, b) for a, b in zip(got[:4], answers[key][:4]) if a is not None))
        else:
            answers[key] = got
        out["device"][name] = t
    set_env({})
    if host_path:
        K = npairs if host_pairs <= 0 else min(host_pairs, npairs)
        read, one, two, same = [], [], [], None
        some = [(i, j) for i in range(D) for j in range(i + 1, D)][:: max(1, npairs // K)][:K]
        for _ in range(repeats):
            t0 = time.perf_counter()
            hist = eng.history_chains(0, W) if hasattr(eng, "history_chains") else eng.history()
            read.append(1e3 * (time.perf_counter() - t0))
            x = hist["x"][1:rows + 1, :W].reshape(N, D)               # rows 1 .. newest of every walker (the ring has not wrapped)
            t0 = time.perf_counter()
            cols = np.ascontiguousarray(x.T)                         # (a feature's sample contiguous: the fast way round)
            h1 = np.stack([np.histogram(cols[f], 20, (lo[f], hi[f]))[0] for f in range(D)])
            one.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            h2 = [np.histogram2d(cols[i], cols[j], 20, [(lo[i], hi[i]), (lo[j], hi[j])])[0] for i, j in some]
            two.append(1e3 * (time.perf_counter() - t0))
            want = answers[(20, True)]
            same = bool(np.array_equal(h1, want[0]) and all(np.array_equal(h.astype(np.int64), want[1][i * D - i * (i + 1) // 2 + (j - i - 1)]) for h, (i, j) in zip(h2, some)))
            print("[histograms_probe] host: read %.0f ms, 1-D %.0f ms, %d pairs %.0f ms, same %s" % (read[-1], one[-1], len(some), two[-1], same), flush=True)
            del hist, x, cols
        measured = [r + a + b for r, a, b in zip(read, one, two)]
        full = [r + a + b * npairs / len(some) for r, a, b in zip(read, one, two)]
        out["host_path"] = {"read_back": spread(read), "np_histogram_every_feature": spread(one), "np_histogram2d_pairs_binned": len(some), "np_histogram2d_those_pairs": spread(two),
                            "counts_equal_the_device's": same, "measured_total (a lower bound of the host path where not every pair was binned)": spread(measured),
                            "total_with_the_pairs_extrapolated_to_all (measured where every pair was binned)": spread(full), "bins": 20}
        one_d = [r + a for r, a in zip(read, one)]
        for name, t in out["device"].items():
            base = one_d if not t["pairs"] else measured
            t["device_slowest_beats_host_fastest"] = t["call_host_clock"]["max_ms"] < min(base)
            t["ratio_host_measured_over_call"] = statistics.median(base) / t["call_host_clock"]["median_ms"]
            if t["pairs"]:
                t["ratio_host_extrapolated_over_call"] = statistics.median(full) / t["call_host_clock"]["median_ms"]
    eng.close()
    return out


def run_step(args):
    shape, _ = STEPS[args.step]
    result = probe_ring(shape, args.repeats, not args.no_host, args.host_pairs if args.step == "large" else 0)
    with open(args.part, "w") as f:
        json.dump(result, f)


def run_probe(args):
    out = {"what": "corner-plot histograms of the cold rung at population shapes (MI355X): ptm_histograms on the device's own history ring against the read-back "
                   "of the ring plus np.histogram / np.histogram2d on the host, and against the walks of a ptm_quantiles call on the same ring "
                   "(tools/histograms_probe.py; a process per step, the repeats of a case in a row; host clock around the calls and stream events; medians with "
                   "the spread).  No hardware counters were collected.",
           "steps": {}}
    with tempfile.TemporaryDirectory() as d:
        for step in args.steps.split(","):
            part = os.path.join(d, step + ".json")
            cmd = ["timeout", "-k", "10", str(STEPS[step][1]), sys.executable, os.path.abspath(__file__), "--step", step, "--part", part, "--repeats", str(args.repeats),
                   "--host-pairs", str(args.host_pairs)]
            if args.no_host:
                cmd.append("--no-host")
            print("[histograms_probe]", " ".join(cmd), flush=True)
            rc = subprocess.call(cmd)
            if rc:
                print("[histograms_probe] step %s ended with status %d: nothing more is started" % (step, rc), flush=True)
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
    ap.add_argument("--steps", default="large,small")
    ap.add_argument("--no-host", action="store_true", help="time the device calls alone")
    ap.add_argument("--host-pairs", type=int, default=3, help="pairs np.histogram2d bins at the large shape (0: all)")
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--step", help="(internal) run one step in this process")
    ap.add_argument("--part", help="(internal) where the step writes its result")
    a = ap.parse_args()
    if a.step:
        run_step(a)
    else:
        sys.exit(run_probe(a))
