"""µs per PT step of a prior ptm_set_prior cannot describe, on the three routes the engine offers, same process, same device, same run:

  (a) host prior + host likelihood   ptm_set_prior_callback + ptm_set_target_callback: the only route such a prior had before
  (b) device likelihood, built-in product prior   ptm_set_target_device alone: the floor (another prior: its chains differ)
  (c) device prior + device likelihood   ptm_set_prior_device + ptm_set_target_device

  python3 tools/device_prior_probe.py [--blocks N] [--out profiles/device_prior.json]

Shapes (dimensions x rungs x walkers): 6 x 20 x 64 and 32 x 64 x 1024.  All three routes run the torch polynomial functions of
tests/device_prior_worker.py (the correlated Gaussian times a hard disc; the polynomial likelihood) -- on route (a) through a host round
trip (numpy -> device -> the function -> numpy).  Per route: a warm-up, a calibration that sizes a block to about 0.3 s, then N >= 5
timed blocks, the routes taken in turn inside every round (a, b, c, a, b, c, ...), each block ended by a device synchronise; reported
is the median with the minimum and the maximum.  torch is imported first (one HIP runtime per process)."""
import argparse
import json
import math
import os
import sys
import time

import torch  # noqa: E402  (before the engine library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from device_prior_worker import disc_prior_torch, host_of, poly_coefs, poly_torch
from ptmcmc_amd import engine as E


def make_engine(D, Nt, W, route):
    rng = np.random.default_rng(11)
    c, k = poly_coefs(D, seed=D)
    beta = E.geometric_ladder(Nt, 1e3)
    blo, bhi, bmin, bmax = [0] * D, [0] * D, [0.0] * D, [0.0] * D
    blo[1], bhi[1], bmin[1], bmax[1] = 3, 3, -2.0, 2.0
    blo[2], bhi[2], bmin[2], bmax[2] = 1, 1, -3.0, 3.0
    x0 = rng.uniform(-1.2, 1.2, size=(Nt * W, D))
    fac = np.tile(np.full(D, 0.6), (Nt, 1)) / np.sqrt(beta)[:, None].clip(1e-2)
    e = E.Engine(D, Nt, W, swap_rate=0.3)
    e.set_bounds(blo, bhi, bmin, bmax)
    like, prior = poly_torch(c, k), disc_prior_torch(D)
    if route == "a":
        e.set_target_callback(host_of(like, D), batched=True)
        e.set_prior_callback(host_of(prior, D), batched=True)
    elif route == "b":
        e.set_prior([1] * D, [0.0] * D, [4.0] * D)
        e.set_target_device(like)
    else:
        e.set_target_device(like)
        e.set_prior_device(prior)
    e.set_ladder(beta)
    e.set_proposals(E.PROP_DIAG, fac, np.full(Nt, 0.2))
    e.set_states(x0)
    return e


def block(e, steps):
    t0 = time.perf_counter()
    e.step(steps); e.sync()
    return (time.perf_counter() - t0) / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_prior.json"))
    a = ap.parse_args()
    if a.blocks < 5:
        raise SystemExit("at least 5 timed blocks")
    if E.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing is measured without one")
    torch.cuda.init()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "unit": "us per PT step", "blocks": a.blocks,
           "method": "host clock around step(n) + sync; routes alternate inside every round; median [min, max] over the blocks", "shapes": []}
    for D, Nt, W in ((6, 20, 64), (32, 64, 1024)):
        engines = {r: make_engine(D, Nt, W, r) for r in "abc"}
        steps, times = {}, {r: [] for r in "abc"}
        for r, e in engines.items():
            block(e, 20)                                          # warm-up: code objects, torch's kernels, the buffers' first touch
            per = block(e, 20)                                    # calibration
            steps[r] = int(min(5000, max(10, math.ceil(0.3e6 / per))))
            block(e, steps[r])                                    # ... and one untimed block of the timed size
        for _ in range(a.blocks):
            for r in "abc":
                times[r].append(block(engines[r], steps[r]))
        row = {"dim": D, "rungs": Nt, "walkers": W, "routes": {}}
        for r, label in (("a", "host prior + host likelihood"), ("b", "device likelihood, built-in product prior"), ("c", "device prior + device likelihood")):
            t = sorted(times[r])
            row["routes"][r] = {"what": label, "median": round(float(np.median(t)), 2), "min": round(t[0], 2), "max": round(t[-1], 2),
                                "steps_per_block": steps[r], "step_kernel": engines[r].step_kernel_name}
        m = {r: row["routes"][r]["median"] for r in "abc"}
        row["c_minus_b"] = round(m["c"] - m["b"], 2)
        row["a_over_c"] = round(m["a"] / m["c"], 2)
        res["shapes"].append(row)
        print("%d x %d x %d: (a) %.1f [%.1f, %.1f]  (b) %.1f [%.1f, %.1f]  (c) %.1f [%.1f, %.1f]  us/step;  (c) - (b) = %.1f, (a) / (c) = %.2f"
              % (D, Nt, W, m["a"], row["routes"]["a"]["min"], row["routes"]["a"]["max"], m["b"], row["routes"]["b"]["min"], row["routes"]["b"]["max"],
                 m["c"], row["routes"]["c"]["min"], row["routes"]["c"]["max"], row["c_minus_b"], row["a_over_c"]), flush=True)
        for e in engines.values():
            e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
