"""µs per PT step of the sampler's ADAPTIVE proposal recipe (--prop_adapt_rate, --prop_adapt_more) drawn on the host (the
host-proposal step) against the same recipe drawn and adapted on the device (ptm_set_proposal_adaptive), same process, same device.

  python3 tools/adaptive_probe.py [--steps N] [--shapes lisa,gauss] [--device-only]

lisa:  examples/example_lisa.cc with the reference's regression flags (--prop_adapt_rate=0.01 --prop_adapt_more) at 20 and 128
       temperatures; host path = PTM_HOST_DE=1.  Per step = the difference of two run lengths over the difference of their steps
       (start-up, initial draws and file writing cancel).
gauss: a 32-dimensional Gaussian, 128 rungs x 512 walkers, the adaptive recipe without differential evolution ({one Gaussian, a
       nested set of six}, rate 0.01 at both levels); host path = the engine's host-proposal callback with numpy draws vectorised over
       the batch and the same adaptation rules vectorised in numpy."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import adaptive_model as AM
from ptmcmc_amd import engine as E
from ptmcmc_amd.problems import GaussianProblem


WHERE = ("host", "device")


def lisa(steps):
    from test_cxx_facade import build
    out = []
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "ex")
        build(exe, "example_lisa.cc")
        for pt in (20, 128):
            for where in WHERE:
                env = dict(os.environ)
                env.pop("PTM_HOST_DE", None)
                if where == "host":
                    env["PTM_HOST_DE"] = "1"
                t = []
                for n in (steps, 3 * steps):
                    t0 = time.perf_counter()
                    r = subprocess.run([exe, "--outname=" + os.path.join(d, "l"), "--pt=%d" % pt, "--nsteps=%d" % n, "--nevery=%d" % steps, "--seed=0.25",
                                        "--prop_adapt_rate=0.01", "--prop_adapt_more"], capture_output=True, text=True, env=env, timeout=3600)
                    t.append(time.perf_counter() - t0)
                    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
                    assert "proposals drawn on the " + where in r.stdout
                us = (t[1] - t[0]) / (2 * steps) * 1e6
                out.append(("lisa %d x 1" % pt, where, us))
                print("lisa %3d x 1  %-6s %9.1f us/step" % (pt, where, us), flush=True)
    return out


def gauss(steps):
    D, Nt, W = 32, 128, 512
    top, inner = [0.3, 0.7], [v / 126.0 for v in (2.0, 4.0, 8.0, 16.0, 32.0, 64.0)]
    scales = [1.0, 1.0] + [2.0 ** -(5 - k) for k in range(6)]
    odfs = [0.5, 0.0] + [0.5] * 6
    out = []
    for where in WHERE:
        pr = GaussianProblem(D, Nt, 1e2)
        eng = E.Engine(D, Nt, W, swap_rate=0.1)
        fac = pr.configure(eng, E.PROP_DIAG)
        eng.init_from_prior()
        cs = AM.ChainSet(top, 0.01, 1, inner, 0.01)
        w, th, bits, cnt = AM.states_of([cs] * (Nt * W))
        if where == "device":
            eng.set_proposal_adaptive(2, np.tile(scales, (Nt, 1)), np.tile(odfs, (Nt, 1)), w, th, bits, cnt, nested=1, K_inner=6, rate=0.01, rate_inner=0.01)
        else:
            S = dict(w=w.copy(), th=th.copy(), last=np.ones((Nt * W, 8), dtype=bool), cnt=cnt.copy(), pick=None)
            sig = np.asarray(fac, dtype=np.float64).reshape(Nt, D)
            rng = np.random.default_rng(1)
            sc, od = np.array(scales), np.array(odfs)

            def propose(X, rung, walker, step):
                c = rung * W + walker
                n = len(c)
                x = rng.uniform(size=n)
                i = np.where(x < S["th"][c, 0], 0, 1)
                xi = rng.uniform(size=n)
                j = np.argmax(xi[:, None] < S["th"][c, 2:], axis=1)
                leaf = np.where(i == 1, 2 + j, 0)
                z = rng.standard_normal((n, D))
                oned = rng.uniform(size=n) < od[leaf]
                ax = rng.integers(0, D, size=n)
                z[oned] = z[oned] * (np.arange(D)[None, :] == ax[oned, None])
                S["pick"] = (c, i, j)
                P = X + sc[leaf, None] * sig[rung] * z
                return P, np.zeros(n), (i + 10 * np.where(i == 1, j + 10 * oned, oned)).astype(np.int32), np.ones(n, dtype=np.int32)

            def result(rung, walker, acc):
                c, i, j = S["pick"]
                a = acc.astype(bool)
                for first, n, m, b in ((0, 2, i, 0), (2, 6, j, 1)):
                    sel = np.ones(len(c), dtype=bool) if b == 0 else i == 1
                    cc, mm, aa = c[sel], m[sel], a[sel]
                    rep = S["last"][cc, first + mm] == aa
                    S["w"][cc[rep], first + mm[rep]] *= 1 - 0.01 * 0.25
                    S["last"][cc, first + mm] = aa
                    S["cnt"][cc, b] += 1
                    rb = cc[S["cnt"][cc, b] >= 10 * n]
                    blk = S["w"][rb, first:first + n]
                    blk /= blk.sum(axis=1, keepdims=True)
                    S["w"][rb, first:first + n] = blk
                    cum = np.cumsum(blk, axis=1)
                    S["th"][rb, first:first + n] = cum / cum[:, -1:]
            eng.set_proposal_callback(propose, result)
        eng.step(3); eng.sync()
        n = steps if where == "device" else max(3, steps // 20)
        t0 = time.perf_counter()
        eng.step(n); eng.sync()
        us = (time.perf_counter() - t0) / n * 1e6
        out.append(("gauss 32-D %d x %d" % (Nt, W), where, us))
        print("gauss 32-D %d x %d  %-6s %9.1f us/step  (%s)" % (Nt, W, where, us, eng.step_kernel_name), flush=True)
        eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--shapes", default="lisa,gauss")
    ap.add_argument("--device-only", action="store_true", help="the device cases alone (e.g. under rocprofv3 --kernel-trace --stats)")
    a = ap.parse_args()
    global WHERE
    if a.device_only:
        WHERE = ("device",)
    res = []
    if "lisa" in a.shapes:
        res += lisa(a.steps)
    if "gauss" in a.shapes:
        res += gauss(a.steps)
    shapes = sorted(set(r[0] for r in res))
    for s in shapes if not a.device_only else []:
        h = [r[2] for r in res if r[0] == s and r[1] == "host"][0]
        d = [r[2] for r in res if r[0] == s and r[1] == "device"][0]
        print("%-24s host %9.1f  device %9.1f us/step  -> %.1fx" % (s, h, d, h / d))


if __name__ == "__main__":
    main()
