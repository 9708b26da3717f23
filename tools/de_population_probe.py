"""Big populations with the reference sampler's default proposal set: what differential evolution on the matrix cores
(de_mfma32_kernel, PTM_DE_MFMA) buys a PT step.  32 dimensions, 128 rungs, W walkers per rung; 80 % differential evolution (snooker
0.1) + six Gaussians with one-dimensional moves at 0.5, evolving ladder 0.01, history of every 100th add, MAP, 10 D = 320 initial rows.

  python tools/de_population_probe.py [--parent DIR] [--out FILE.json] [--shapes 512,1024,4096] [--steps 300] [--warmup 30] [--repeats 5]

For every shape one child process per leg -- PTM_DE_MFMA=0, PTM_DE_MFMA=1 and, with --parent DIR, the build of another checkout (its
ptmcmc_amd package with its own library; the switch means nothing to an older one) -- because the engine reads the switch once.  Each
child runs under `timeout`, and the run stops at the first child that fails.  A child times `repeats` batches of `steps` PT steps
after `warmup`; the record holds min / median / max of the batches in us per step and MH steps per second.  The ring (100 rows) and
the initial rows take 27 KB per chain: 7, 14 and 56 GB of device memory at W = 512, 1024, 4096.

  python tools/de_population_probe.py child TREE W steps warmup repeats      (one leg; prints one JSON line)"""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, NT, EVERY, CAP = 32, 128, 100, 100


def child(tree, W, steps, warm, reps):
    sys.path.insert(0, os.path.abspath(tree))
    import numpy as np
    from ptmcmc_amd import engine as E
    from ptmcmc_amd.problems import GaussianProblem
    assert 2 * (warm + reps * steps) // EVERY + 2 <= CAP, "the ring must hold every row of the run"
    pr = GaussianProblem(D, NT, 1e6)
    e = E.Engine(D, NT, W, add_every_n=EVERY, history_rungs=NT, history_capacity=CAP, map_rungs=NT)
    pr.configure(e, E.PROP_DIAG)
    K = 6
    g = 2.0 ** np.arange(1, K + 1)
    shares = np.concatenate([[0.8], 0.2 * g / g.sum()])
    cum = np.tile(np.cumsum(shares), (NT, 1)); cum[:, -1] = 1.0
    scales = np.tile(np.concatenate([[-1.0], 4.0 ** -np.arange(K)[::-1]]), (NT, 1))
    odfs = np.tile(np.concatenate([[0.0], np.full(K, 0.5)]), (NT, 1))
    e.set_proposal_mixture(cum, scales, odfs)
    e.init_from_prior()
    # initial rows: one random block of 4096 chains, repeated over the population (43 GB of fresh random numbers would take minutes)
    rng = np.random.default_rng(1)
    nb = min(4096, NT * W)
    block = rng.uniform(-1.0, 1.0, size=(10 * D, nb, D)) * np.asarray(pr.halfwidths)[None, None, :] * 0.02
    init = np.tile(block, (1, NT * W // nb, 1))
    assert init.shape == (10 * D, NT * W, D)
    e.set_proposal_de(0.1, 0.3, 4.0, 0.0, init_rows=init)
    del init, block
    e.set_evolve_temps(0.01)
    e.step(warm); e.sync()
    us = []
    for _ in range(reps):
        t0 = time.perf_counter()
        e.step(steps); e.sync()
        us.append((time.perf_counter() - t0) / steps * 1e6)
    t, a = e.counter_sums()
    lt = np.unique(e.last_type)
    print(json.dumps(dict(W=W, chains=NT * W, us_per_step=us, step_kernel=e.step_kernel_name, mh_acceptance=a / max(1, t),
                          de_types_accepted=bool(((lt == 0) | (lt == 10)).any()))), flush=True)
    e.close()


def summary(us, chains):
    s = sorted(us)
    mid = s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])
    return dict(us_per_step=dict(min=round(s[0], 2), median=round(mid, 2), max=round(s[-1], 2)),
                mh_steps_per_s=dict(min=round(chains / s[-1] * 1e6), median=round(chains / mid * 1e6), max=round(chains / s[0] * 1e6)))


def main(argv):
    opt = dict(parent=None, out=None, shapes="512,1024,4096", steps="300", warmup="30", repeats="5")
    while argv:
        k = argv.pop(0)
        assert k.startswith("--") and k[2:] in opt and argv, __doc__
        opt[k[2:]] = argv.pop(0)
    legs = ([("parent", opt["parent"], None)] if opt["parent"] else []) + [("PTM_DE_MFMA=0", HERE, "0"), ("PTM_DE_MFMA=1", HERE, "1")]
    rec = dict(config=dict(D=D, rungs=NT, add_every_n=EVERY, history_capacity=CAP, initial_rows=10 * D, steps=int(opt["steps"]), warmup=int(opt["warmup"]),
                           repeats=int(opt["repeats"]), recipe="DE 0.8 (snooker 0.1), six Gaussians, one-dimensional moves 0.5, evolving ladder 0.01"),
               shapes={})
    for W in (int(v) for v in opt["shapes"].split(",")):
        row = {}
        for name, tree, switch in legs:
            env = dict(os.environ)
            env.pop("PTM_DE_MFMA", None)
            env.pop("PTM_ENGINE_LIB", None)
            if switch is not None:
                env["PTM_DE_MFMA"] = switch
            limit = 120 + W // 8   # seconds: the initial rows of the biggest shape are 43 GB on their way through the host
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "child", tree, str(W), opt["steps"], opt["warmup"], opt["repeats"]]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if r.returncode != 0:
                print("W=%d %s: the child failed (%d) -- stopping\n%s\n%s" % (W, name, r.returncode, r.stdout[-2000:], r.stderr[-3000:]), flush=True)
                return 1
            c = json.loads(r.stdout.strip().splitlines()[-1])
            row[name] = dict(summary(c["us_per_step"], c["chains"]), step_kernel=c["step_kernel"], mh_acceptance=round(c["mh_acceptance"], 4),
                             de_types_accepted=c["de_types_accepted"], batches_us_per_step=[round(v, 2) for v in c["us_per_step"]])
            print("W=%d %-14s %s  %s" % (W, name, row[name]["us_per_step"], c["step_kernel"]), flush=True)
        rec["shapes"]["W=%d" % W] = row
        if opt["out"]:   # (after every shape: a later failure leaves what was measured)
            with open(opt["out"], "w") as fh:
                json.dump(rec, fh, indent=1)
                fh.write("\n")
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child(sys.argv[2], *(int(v) for v in sys.argv[3:8]))
    else:
        sys.exit(main(sys.argv[1:]))
