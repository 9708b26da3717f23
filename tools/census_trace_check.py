#!/usr/bin/env python3
"""Did every build of the census really run?  Reads kernel statistics recorded with rocprofv3 --kernel-trace --stats of
tests/test_gpu_build_census.py (profiles/build_census_kernel_stats.csv, and build_census_force_valu_kernel_stats.csv of its child
process) and tests/build_census.py's CASES; fails unless every name of
the table appears among the traced kernels with at least one call.

usage: python tools/census_trace_check.py [stats.csv ...]     (default: profiles/build_census*_kernel_stats.csv)"""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import build_census as BC


def calls_by_name(paths):
    """{the engine's name of a traced kernel: calls}, summed over the files (build_census.reported_name)"""
    calls = {}
    for path in paths:
        with open(path, newline="") as fh:
            rows = csv.DictReader(ln for ln in fh if not ln.startswith("#"))
            for row in rows:
                name = BC.reported_name(row["Name"])
                if name:
                    calls[name] = calls.get(name, 0) + int(row["Calls"])
    return calls


def main(argv):
    paths = argv or sorted(glob.glob(os.path.join(ROOT, "profiles", "build_census*_kernel_stats.csv")))
    calls = calls_by_name(paths)
    missing = [n for n in sorted(BC.CASES) if calls.get(n, 0) < 1]
    for n in missing:
        print("never launched: %s   (%s)" % (n, BC.key(BC.CASES[n])))
    print("%d of %d census builds appear in %s" % (len(BC.CASES) - len(missing), len(BC.CASES), ", ".join(os.path.relpath(p, ROOT) for p in paths)))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
