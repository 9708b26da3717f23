"""Which kernels does an engine of a given configuration run?  Records ptm_sweep_kernel_name / ptm_step_kernel_name of a fixed list of
configurations in tests/golden/kernel_names.json; tests/test_gpu_kernel_names.py holds every later tree to the recorded names.

Only the public Python API is used, engines are configured and never stepped.  The engine reads its environment switches once per
process, so each environment variant names its configurations in a child process of its own (--variant NAME prints them as JSON).

usage: python tests/golden/make_kernel_names.py            (needs the built engine and an MI355X; rewrites kernel_names.json)"""
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "kernel_names.json")


def cfg(D, Nt, W, kind="lower", **opts):
    """opts: bounds ("limit" / "wrap"), gauss_prior, mean, oned, mix, evolve ("rate" / "cut"), hist, de, ada, host_prop, host_like,
    dev_like, time_kernels, shard (the local rung count of a rung shard that begins at rung 0)"""
    c = dict(D=D, Nt=Nt, W=W, kind=kind)
    c.update(opts)
    return c


def key(c):
    parts = ["D%d %dx%d %s" % (c["D"], c["Nt"], c["W"], c["kind"])]
    for k in sorted(c):
        if k in ("D", "Nt", "W", "kind") or not c[k]:
            continue
        parts.append(k if c[k] is True else "%s=%s" % (k, c[k]))
    return " ".join(parts)


CONFIGS = (
    # every padded dimension, whole waves per rung, the plain workload
    [cfg(D, 8, 64) for D in (2, 6, 12, 21, 32, 48, 64, 100, 128, 200)]
    # one walker per rung: the latency regime
    + [cfg(D, 20, 1) for D in (2, 12, 32, 64, 200)]
    + [cfg(32, 256, 4), cfg(12, 256, 4, "diag")]
    # walkers that do not fill waves
    + [cfg(D, 4, 63) for D in (6, 21, 48, 100)]
    # more than 4096 such chains: past the lane-per-dimension kernel at 4 padded dimensions
    + [cfg(2, 66, 63), cfg(2, 66, 63, ada=True)]
    # 32 dimensions, whole waves per rung: the matrix-core builds and what keeps a workload off them
    + [cfg(32, 16, 320, k) for k in ("lower", "dense", "diag")]
    + [cfg(32, 16, 320, **o) for o in (
        dict(bounds="limit"), dict(bounds="wrap"), dict(gauss_prior=True), dict(mean=True), dict(oned=True), dict(mix=True),
        dict(evolve="rate"), dict(evolve="cut"), dict(hist=True), dict(hist=True, bounds="limit"), dict(hist=True, gauss_prior=True),
        dict(evolve="rate", bounds="limit"), dict(evolve="rate", hist=True), dict(evolve="rate", hist=True, mean=True),
        dict(de=True), dict(ada=True), dict(host_prop=True), dict(host_like=True), dict(dev_like=True), dict(time_kernels=True))]
    # ... and populations big enough for the compacted sweep
    + [cfg(32, 2, 1024, **o) for o in (
        dict(), dict(bounds="limit"), dict(bounds="limit", mean=True), dict(bounds="limit", evolve="rate"),
        dict(bounds="limit", mix=True, evolve="rate"), dict(evolve="rate"), dict(hist=True), dict(bounds="wrap"), dict(oned=True))]
    + [cfg(21, 2, 1024, "dense"), cfg(32, 4, 1024, shard=2), cfg(6, 2, 1024), cfg(12, 2, 1024)]
    # 33..128 dimensions: the matrix-core builds' flags, and the lanes kernel for the rest
    + [cfg(D, 8, 64, **o) for D in (64, 128) for o in (dict(bounds="limit"), dict(evolve="rate"), dict(bounds="limit", evolve="rate"))]
    + [cfg(48, 8, 64, "dense"), cfg(64, 8, 64, hist=True), cfg(64, 8, 64, mean=True), cfg(100, 8, 64, bounds="wrap"), cfg(48, 8, 64, ada=True)]
    # the persistent ladder kernel's builds
    + [cfg(2, 8, 64, **o) for o in (
        dict(oned=True), dict(hist=True), dict(evolve="rate"), dict(evolve="rate", mix=True), dict(de=True), dict(de=True, evolve="rate"),
        dict(bounds="wrap"), dict(bounds="wrap", evolve="rate"), dict(bounds="wrap", de=True), dict(gauss_prior=True, de=True, evolve="rate"),
        dict(evolve="cut"), dict(time_kernels=True), dict(host_like=True))]
    + [cfg(2, 8, 64, "diag"), cfg(6, 1, 64), cfg(12, 16, 320, evolve="cut")]
    # differential evolution and adaptive sets on either side of the lanes kernel's rule
    + [cfg(12, 16, 320, de=True, time_kernels=True), cfg(6, 16, 320, de=True, time_kernels=True), cfg(12, 4, 63, ada=True), cfg(12, 16, 320, ada=True),
       cfg(12, 4, 63, host_prop=True), cfg(6, 4, 63, host_like=True), cfg(6, 4, 63, dev_like=True)]
)

VARIANTS = {
    "PTM_FORCE_VALU=1": [cfg(32, 16, 320), cfg(32, 2, 1024), cfg(32, 2, 1024, bounds="limit"), cfg(64, 8, 64), cfg(128, 8, 64), cfg(32, 4, 63),
                         cfg(32, 16, 320, de=True), cfg(12, 16, 320, de=True, time_kernels=True)],
    "PTM_COMPACT=0": [cfg(32, 2, 1024), cfg(32, 2, 1024, bounds="limit"), cfg(32, 2, 1024, bounds="limit", mean=True), cfg(32, 2, 1024, evolve="rate")],
    "PTM_FUSED=0": [cfg(2, 8, 64), cfg(6, 1, 64), cfg(2, 8, 64, evolve="cut"), cfg(12, 2, 1024)],
    "PTM_LADDER=0": [cfg(2, 8, 64), cfg(12, 16, 320), cfg(32, 256, 4), cfg(6, 8, 64, evolve="rate"), cfg(12, 16, 320, evolve="rate"), cfg(2, 8, 64, hist=True)],
}


def names_of(c):
    """the engine of one configuration, configured and not stepped: [sweep_kernel_name, step_kernel_name]"""
    import numpy as np
    from ptmcmc_amd import engine as E
    from ptmcmc_amd.problems import GaussianProblem
    D, Nt, W = c["D"], c["Nt"], c["W"]
    nloc = c.get("shard") or Nt
    hist = c.get("hist") or c.get("de")
    kw = dict(history_rungs=nloc, history_capacity=16, map_rungs=nloc) if hist else {}
    eng = E.Engine(D, Nt, W, swap_rate=0.1, rung_begin=0, rung_count=nloc, time_kernels=bool(c.get("time_kernels")), **kw)
    pr = GaussianProblem(D, Nt, 1e3)
    lo, hi = pr.centers - pr.halfwidths, pr.centers + pr.halfwidths
    b = {None: E.BOUND_OPEN, "limit": E.BOUND_LIMIT, "wrap": E.BOUND_WRAP}[c.get("bounds")]
    eng.set_bounds([b] * D, [b] * D, lo, hi)
    eng.set_prior([E.PRIOR_GAUSSIAN if c.get("gauss_prior") else E.PRIOR_UNIFORM] * D, pr.centers, pr.halfwidths)
    eng.set_target_gaussian(pr.P, pr.like0, mean=np.full(D, 0.25) if c.get("mean") else None)
    keep = []
    if c.get("host_like"):
        eng.set_target_callback(lambda x: 0.0)
    if c.get("dev_like"):
        fn = E.LOGLIKE_DEVICE_FN(lambda *a: None)
        keep.append(fn)
        eng.set_target_device_c(C.cast(fn, C.c_void_p))
    eng.set_ladder(pr.beta)
    kind = {"lower": E.PROP_LOWER, "dense": E.PROP_DENSE, "diag": E.PROP_DIAG}[c["kind"]]
    f = pr.proposal_factors(range(nloc), lower=(kind != E.PROP_DENSE))
    if kind == E.PROP_DIAG:
        f = np.stack([np.sqrt(np.diag(T @ T.T)) for T in f])
    eng.set_proposals(kind, f, np.full(nloc, 0.5) if c.get("oned") else None)
    if c.get("mix") or c.get("de"):
        scales = [-1.0, 1.0] if c.get("de") else [1.0, 0.5]
        eng.set_proposal_mixture(np.tile([0.5, 1.0], (nloc, 1)), np.tile(scales, (nloc, 1)), np.zeros((nloc, 2)))
    if c.get("de"):
        eng.set_proposal_de(0.1, 0.3, 4.0, 0.0)
    if c.get("ada"):
        Nc = nloc * W
        eng.set_proposal_adaptive(2, np.tile([1.0, 0.5], (nloc, 1)), np.zeros((nloc, 2)), np.full((Nc, 2), 0.5), np.tile([0.5, 1.0], (Nc, 1)), rate=0.01)
    if c.get("host_prop"):
        eng.set_proposal_callback(lambda X, r, w, s: (X, np.zeros(len(X)), np.zeros(len(X), dtype=np.int32), np.ones(len(X), dtype=np.int32)))
    if c.get("evolve"):
        eng.set_evolve_temps(0.01, 5.0 if c["evolve"] == "cut" else -1.0)
    out = [eng.sweep_kernel_name, eng.step_kernel_name]
    eng.close()
    return out


def variant_names(variant):
    """the names of a variant's configurations, from a child process that has the variant's switch in its environment"""
    name, value = variant.split("=")
    env = dict(os.environ)
    env[name] = value
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", variant], env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError("%s: child process failed (%d)\n%s\n%s" % (variant, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main(argv):
    sys.path.insert(0, ROOT)
    if len(argv) == 2 and argv[0] == "--variant":
        print(json.dumps({"%s | %s" % (argv[1], key(c)): names_of(c) for c in VARIANTS[argv[1]]}))
        return
    names = {key(c): names_of(c) for c in CONFIGS}
    for v in VARIANTS:
        names.update(variant_names(v))
    with open(OUT, "w") as fh:
        json.dump(names, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("wrote %d entries to %s" % (len(names), OUT))


if __name__ == "__main__":
    main(sys.argv[1:])
