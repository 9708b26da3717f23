"""µs per PT step of a user likelihood evaluated on the host (ptm_set_target_callback) against the same likelihood on the device
(ptm_set_target_device), same process, same device, same run.

  python3 tools/device_likelihood_probe.py [--steps N] [--shapes lisa,gauss]

Shapes: the toy LISA likelihood (exampleLISA.cc:59-72,130-142) at 20 x 1, 128 x 1, 20 x 64 and 20 x 1024 (rungs x walkers) with the
sampler's default recipe (differential evolution 0.8 + six Gaussians, evolving ladder, history, MAP); a 32-dimensional Gaussian at
128 x 512.  Device: the HIP kernel of examples/lisa_device_likelihood.hip (built here with hipcc) through set_target_device_c; the
Gaussian as a torch function through set_target_device.  Host: numpy, vectorised over the batch, through the Python binding's
callback.  torch is imported first (one HIP runtime per process)."""
import argparse
import ctypes as C
import math
import os
import subprocess
import sys
import tempfile
import time

import torch  # noqa: E402  (before the engine library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import lisa_toy
from ptmcmc_amd import engine as E

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def lisa_numpy(X):
    d, phi, inc, lam, beta, psi = (X[:, j] for j in range(6))
    ap = 1j * (0.75 * (3 - np.cos(2 * beta)) * np.cos(2 * lam - math.pi / 3))
    ac = 1j * (3.0 * np.sin(beta) * np.sin(2 * lam - math.pi / 3))
    ep = -1j * (0.75 * (3 - np.cos(2 * beta)) * np.sin(2 * lam - math.pi / 3))
    ec = 1j * (3.0 * np.sin(beta) * np.cos(2 * lam - math.pi / 3))
    pref = 0.5 / d * math.sqrt(5 / math.pi)
    def modes(p, c):
        return (pref * np.cos(inc / 2) ** 4 * np.exp(2j * (-phi - psi)) * 0.5 * (p + 1j * c)
                + pref * np.sin(inc / 2) ** 4 * np.exp(2j * (-phi + psi)) * 0.5 * (p - 1j * c))
    sa, se = modes(ap, ac), modes(ep, ec)
    return -0.5 * lisa_toy.FACTOR * (np.abs(sa - lisa_toy.SA_INJ) ** 2 + np.abs(se - lisa_toy.SE_INJ) ** 2)


def recipe(Nt, K=6, de_share=0.8, odf=0.5):
    g = 2.0 ** np.arange(1, K + 1)
    shares = np.concatenate([[de_share], (1 - de_share) * g / g.sum()])
    cum = np.tile(np.cumsum(shares), (Nt, 1)); cum[:, -1] = 1.0
    scales = np.tile(np.concatenate([[-1.0], 2.0 ** -np.arange(K)[::-1]]), (Nt, 1))
    odfs = np.tile(np.concatenate([[0.0], np.full(K, odf)]), (Nt, 1))
    return cum, scales, odfs


def lisa_engine(Nt, W, target, hist):
    D = 6
    beta = E.geometric_ladder(Nt, 1e9)
    sig = np.array(lisa_toy.SCALES) / 20.0
    e = E.Engine(D, Nt, W, swap_rate=0.1, history_rungs=Nt, history_capacity=hist, map_rungs=Nt)
    e.set_bounds(lisa_toy.BLO, lisa_toy.BHI, lisa_toy.BMIN, lisa_toy.BMAX)
    e.set_prior(lisa_toy.TYPES, lisa_toy.CENTERS, lisa_toy.SCALES)
    target(e)
    e.set_ladder(beta)
    e.set_proposals(E.PROP_DIAG, np.tile(sig, (Nt, 1)) / np.sqrt(beta)[:, None].clip(1e-3), np.full(Nt, 0.5))
    e.init_from_prior()
    cum, scales, odfs = recipe(Nt)
    e.set_proposal_mixture(cum, scales, odfs)
    e.set_proposal_de(0.1, 0.3, 4.0, 0.0)
    e.set_evolve_temps(0.01)
    return e


def gauss_engine(D, Nt, W, target):
    from ptmcmc_amd.problems import GaussianProblem
    pr = GaussianProblem(D, Nt, 1e3)
    e = E.Engine(D, Nt, W, swap_rate=0.1)
    pr.configure(e, E.PROP_LOWER)
    target(e, pr)
    e.init_from_prior()
    return e


def time_steps(e, steps, warm):
    e.step(warm); e.sync()
    t0 = time.perf_counter()
    e.step(steps); e.sync()
    return (time.perf_counter() - t0) / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--shapes", default="lisa,gauss")
    a = ap.parse_args()
    torch.cuda.init()
    dev = torch.device("cuda", 0)
    print("device: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__), flush=True)
    rows = []
    with tempfile.TemporaryDirectory() as d:
        if "lisa" in a.shapes:
            so = os.path.join(d, "liblisa_device.so")
            subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                                   os.path.join(ROOT, "examples", "lisa_device_likelihood.hip"), "-o", so])
            lib = C.CDLL(so)
            fp = C.cast(lib.lisa_loglike_device, C.c_void_p).value
            for Nt, W in ((20, 1), (128, 1), (20, 64), (20, 1024)):
                steps = a.steps if Nt * W <= 2560 else max(20, a.steps // 10)
                hist = steps + 80
                eh = lisa_engine(Nt, W, lambda e: e.set_target_callback(lisa_numpy, batched=True), hist)
                th = time_steps(eh, steps, 10)
                nh = eh.step_kernel_name
                eh.close()
                ed = lisa_engine(Nt, W, lambda e: e.set_target_device_c(fp), hist)
                td = time_steps(ed, steps, 10)
                nd = ed.step_kernel_name
                ed.close()
                rows.append(("toy LISA, default recipe", Nt, W, th, td, nh, nd))
                print("toy LISA %4d x %4d: host callback %9.1f us/step   device %8.1f us/step   (x%.1f)   [%s | %s]"
                      % (Nt, W, th, td, th / td, nh, nd), flush=True)
        if "gauss" in a.shapes:
            D, Nt, W = 32, 128, 512
            steps = max(20, a.steps // 10)
            holder = {}

            def host_t(e, pr):
                P = np.asarray(pr.P)
                e.set_target_callback(lambda X: pr.like0 - 0.5 * np.einsum("ij,jk,ik->i", X, P, X), batched=True)

            def dev_t(e, pr):
                P = torch.as_tensor(np.asarray(pr.P), device=dev)
                holder["P"] = P

                def f(X, count, out):
                    out.copy_(pr.like0 - 0.5 * ((X @ P) * X).sum(1))
                e.set_target_device(f)
            eh = gauss_engine(D, Nt, W, host_t)
            th = time_steps(eh, steps, 3)
            nh = eh.step_kernel_name
            eh.close()
            ed = gauss_engine(D, Nt, W, dev_t)
            td = time_steps(ed, steps, 3)
            nd = ed.step_kernel_name
            ed.close()
            rows.append(("32-D Gaussian (torch on the device, numpy on the host)", Nt, W, th, td, nh, nd))
            print("Gaussian D=32 %4d x %4d: host callback %9.1f us/step   device %8.1f us/step   (x%.1f)   [%s | %s]"
                  % (Nt, W, th, td, th / td, nh, nd), flush=True)
    print("\n| workload | rungs x walkers | host callback (us/step) | device likelihood (us/step) | ratio |")
    print("|---|---|---|---|---|")
    for name, Nt, W, th, td, _, _ in rows:
        print("| %s | %d x %d | %.1f | %.1f | %.1f |" % (name, Nt, W, th, td, th / td))


if __name__ == "__main__":
    main()
