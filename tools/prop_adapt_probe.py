"""ptm_adapt_proposals (every rung's Gaussian factor from its own samples, moments and eigen-decompositions on the device) against the
host route (ptm_moments per rung, the facade's gaussian_prop::eigen_factor on one core, ptm_set_proposal_rung per rung), alternating in
one process, at 6 dimensions x 20 rungs x 64 walkers x 1000 rows and 32 x 128 x 1024 x 64.  Times are host clocks around calls that end in
a wait for the stream; medians of --repeats runs with minimum and maximum.  The device call's legs: ptm_moments_rungs alone,
ptm_eigen_factors alone on the same covariances (it carries their copy to the device and the factors' copy back, which the whole call
does not pay), the install by difference.  Both routes must give the same factors, bit for bit.
usage: python tools/prop_adapt_probe.py [--repeats 5] [--out profiles/proposal_adapt.json] [--shapes small,large]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ptmcmc_amd import engine as E
from ptmcmc_amd.problems import GaussianProblem

SHAPES = {"small": (6, 20, 64, 1000), "large": (32, 128, 1024, 64)}


def host_eigen_lib(d):
    so = os.path.join(d, "libhost_eigen.so")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ptmcmc_amd", "host"),
                           os.path.join(ROOT, "tools", "prop_adapt_host_eigen.cc"), "-pthread", "-o", so])
    lib = C.CDLL(so)
    lib.host_eigen_factors.argtypes = [E._dp, C.c_int, C.c_int, C.c_double, E._dp, E._i32p]
    lib.host_eigen_factors.restype = None
    return lib


def clock(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs": len(v)}


def probe(name, lib, repeats):
    D, Nt, W, rows = SHAPES[name]
    scale = 2.38 / np.sqrt(D)
    eng = E.Engine(D, Nt, W, seed=0x5EEDAD09, swap_rate=0.1, history_rungs=Nt, history_capacity=rows + 8)
    GaussianProblem(D, Nt, 1e2).configure(eng, E.PROP_DENSE)
    eng.init_from_prior()
    eng.step(rows)
    eng.sync()
    t = {k: [] for k in ("device_total", "device_moments", "device_eigen", "device_install_by_difference", "host_total", "host_moments", "host_eigen", "host_install")}

    def device():
        tt, (status, fac) = clock(lambda: eng.adapt_proposals(nrows=rows, scale=scale, factors=True))
        tm, mom = clock(lambda: eng.moments_rungs(nrows=rows))
        te, _ = clock(lambda: E.eigen_factors(mom[1]))
        return tt, tm, te, status, fac

    def host():
        tm, covs = clock(lambda: np.stack([eng.posterior_moments(r, D, rows)[1] for r in range(Nt)]))
        fac, status = np.empty((Nt, D, D)), np.empty(Nt, dtype=np.int32)
        te, _ = clock(lambda: lib.host_eigen_factors(E._d(covs), Nt, D, scale, E._d(fac), status.ctypes.data_as(E._i32p)))

        def install():
            for r in range(Nt):
                if status[r] == 0:
                    eng.set_proposal_rung(r, fac[r])
            eng.sync()
        ti, _ = clock(install)
        return tm, te, ti, status, fac

    device(), host()                                   # warm-up of every leg at this shape
    same = True
    for _ in range(repeats):                           # alternating
        tt, tm, te, sd, fd = device()
        hm, he, hi, sh, fh = host()
        same = same and np.array_equal(sd, sh) and fd.tobytes() == fh.tobytes()
        for k, v in (("device_total", tt), ("device_moments", tm), ("device_eigen", te), ("device_install_by_difference", tt - tm - te),
                     ("host_total", hm + he + hi), ("host_moments", hm), ("host_eigen", he), ("host_install", hi)):
            t[k].append(v)
    res = {"shape": {"dim": D, "rungs": Nt, "walkers": W, "rows": rows}, "rungs_set": int((sd == 0).sum()), "same_factors_bit_for_bit": bool(same),
           "sweep_kernel": eng.sweep_kernel_name}
    res.update({k: stats(v) for k, v in t.items()})
    res["device_over_host"] = res["device_total"]["median_ms"] / res["host_total"]["median_ms"]
    eng.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proposal_adapt.json"))
    ap.add_argument("--shapes", default="small,large")
    a = ap.parse_args()
    if E.device_count() < 1:
        raise SystemExit("prop_adapt_probe: no gfx950 device visible (a timing needs the GPU)")
    with tempfile.TemporaryDirectory() as d:
        lib = host_eigen_lib(d)
        out = {"what": "ptm_adapt_proposals against the host route (ptm_moments per rung + gaussian_prop::eigen_factor on one core + ptm_set_proposal_rung per rung); "
                       "host clocks around calls that end in a wait; device_eigen is ptm_eigen_factors alone and carries copies the whole call does not pay, "
                       "so device_install_by_difference is a lower estimate", "repeats": a.repeats}
        for name in a.shapes.split(","):
            out[name] = probe(name, lib, a.repeats)
            print(name, json.dumps(out[name]), flush=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("written to", a.out)
