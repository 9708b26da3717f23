"""The census of kernel builds: one configuration for every sweep and step kernel of the gfx950 code objects, chosen so that the
engine runs exactly that build.  A plain table (no GPU, no engine library): tests/test_build_census_cpu.py holds it to the kernels
that were built and to the sweep plan, tests/test_gpu_build_census.py steps every configuration against the checker,
tools/census_trace_check.py holds a recorded kernel trace of that run to it.

CASES[name] is a configuration in the style of tests/golden/make_kernel_names.py's cfg:
  D, Nt, W, kind ("lower" / "dense" / "diag")
  bounds        "limit": open / limit boundaries, narrow, on a few dimensions;  "wrap": wrap, reflect and limit boundaries
  gauss_prior   Gaussian prior factors on some dimensions (with bounds="wrap" this is the general state space)
  mean          a target mean
  oned          the fraction of one-dimensional moves
  mix           the members of a scale mixture
  evolve        the rate of evolving ladders
  hist          history and MAP of every hist-th add (every add beside differential evolution or an adaptive set)
  de            differential evolution (a member of the set, drawn from initial rows and the history)
  ada           an adaptive proposal set of three Gaussians (rate 0.3)
  time_kernels  the engine times its kernels: its PT steps stay on the two-launch path (exchange kernel + sweep kernel)
  env           an environment switch of the engine ("PTM_FORCE_VALU=1"): the case runs in a child process that has it
Every case's build is launched by step(), after real exchange phases: step_kernel_name is "decide_kernel + " + name for a sweep
build (time_kernels, or a population too big for the step kernels, sees to that) and the name itself for the two step kernels; the
compacted names are met by step() only.

Shapes are the smallest at which the build can still go wrong: D = DP - 3 (D = 3 at DP 4), so that every build has padded lanes;
3 to 6 rungs; 64 walkers for whole-wave builds (128 once per matrix-core family: a second wave per rung), 3 or 5 for the lanes builds,
1024 x 3 rungs for the compacted builds, four chains (a ladder of four rungs) from 256 padded dimensions up.  Exceptions, each forced by the engine's rule
for the build: the lane-per-chain kernel takes a population that does not fill waves only past 4096 chains (821 x 5) at 4 and 8
padded dimensions and only with PTM_FORCE_VALU=1 at 16 and 32 (short of 65536 chains); the small-ladder step kernel is met past the
persistent kernel's 1024 workgroups (1088 walkers), its 256-thread form from rungs x DP > 64 on (17, 9 and 5 rungs); the
persistent kernel's builds with everything (7, 15, 31) run ladders of two workgroups, the second ragged, and its builds of the general
state space without differential evolution (19, 23) 64 walkers, since they accept little beyond their coldest rungs."""

import re

DPS = (4, 8, 16, 32, 64, 128, 256, 512, 1024)
FAMILIES = ("sweep_", "ladder_persistent_kernel<", "ladder_steps_kernel<")


def reported_name(symbol):
    """the engine's name for a demangled kernel symbol ("void ptm::NAME(arguments)", as nm | c++filt or a kernel trace prints it), or None
    if it is no sweep or step kernel; the engine's name of sweep_kernel leaves the last, defaulted argument out unless it is set"""
    m = re.match(r"(?:void )?ptm::(.*>)\(", symbol)
    if not m or not m.group(1).startswith(FAMILIES):
        return None
    return re.sub(r"^(sweep_kernel<\d+, \d, \w+, \w+), false>$", r"\1>", m.group(1))


KIND_NAME = {0: "dense", 1: "diag", 2: "lower"}
FORCE_VALU = "PTM_FORCE_VALU=1"


def dim_of(DP):
    return 3 if DP == 4 else DP - 3


def padded(D):
    for DP in DPS:
        if D <= DP:
            return DP
    raise ValueError(D)


def cfg(D, Nt, W, kind="lower", **opts):
    c = dict(D=D, Nt=Nt, W=W, kind=kind)
    c.update(opts)
    return c


def tf(v):
    return "true" if v else "false"


# what makes a build "general" (not the plain workload), in turn: every feature meets several builds
FEATURES = (dict(oned=0.4), dict(bounds="limit"), dict(bounds="wrap", gauss_prior=True), dict(mean=True, mix=2), dict(evolve=0.03, hist=2), dict(bounds="limit", oned=0.3, evolve=0.02),
            dict(gauss_prior=True, mix=3, hist=1))

CASES = {}


def _add(name, c):
    assert name not in CASES, name
    if c.get("ada"):   # (the adaptive set is the proposal set: no fixed mixture, no one-dimensional fraction of the base proposal beside it)
        c.pop("mix", None); c.pop("oned", None)
    CASES[name] = c


def _sweep_kernel_cases():
    """sweep_kernel<DP, KIND, UNI, SIMPLE, ADA>: a lane walks a chain"""
    n = 0
    for DP in (4, 8, 16, 32):
        D = dim_of(DP)
        for k in (0, 1, 2):
            kind = KIND_NAME[k]
            # whole waves per rung: 32 dimensions belong to the matrix cores unless the switch keeps them off
            uni = dict(env=FORCE_VALU) if DP == 32 else {}
            _add("sweep_kernel<%d, %d, true, true>" % (DP, k), cfg(D, 4, 64, kind, time_kernels=True, **uni))
            _add("sweep_kernel<%d, %d, true, false>" % (DP, k), cfg(D, 5, 64, kind, time_kernels=True, **uni, **FEATURES[n % len(FEATURES)]))
            # (an adaptive set keeps every dimension off the matrix cores)
            _add("sweep_kernel<%d, %d, true, false, true>" % (DP, k), cfg(D, 4, 64, kind, ada=True, time_kernels=True, **FEATURES[(n + 2) % len(FEATURES)]))
            # walkers that do not fill waves: past the lanes kernel's 4096 chains (4, 8), or with the switch
            odd = dict(Nt=5, W=821) if DP <= 8 else dict(Nt=5, W=5, env=FORCE_VALU)
            _add("sweep_kernel<%d, %d, false, false>" % (DP, k),
                 cfg(D, odd["Nt"], odd["W"], kind, time_kernels=True, **({"env": odd["env"]} if "env" in odd else {}), **FEATURES[(n + 1) % len(FEATURES)]))
            odd_ada = dict(Nt=5, W=821) if DP <= 8 else dict(Nt=4, W=3, env=FORCE_VALU)
            _add("sweep_kernel<%d, %d, false, false, true>" % (DP, k),
                 cfg(D, odd_ada["Nt"], odd_ada["W"], kind, ada=True, time_kernels=True, **({"env": odd_ada["env"]} if "env" in odd_ada else {}),
                     **(FEATURES[(n + 3) % len(FEATURES)] if DP > 8 else {})))
            n += 1


def _lanes_cases():
    """sweep_lanes_kernel<DP, KIND, GEN> and sweep_lanes_ada_kernel<DP, KIND>: a lane per dimension"""
    n = 0
    for DP in DPS:
        D = dim_of(DP)
        Nt, W = (5, 3) if DP <= 128 else (4, 1)
        tk = dict(time_kernels=True) if DP <= 32 else {}   # (up to 32 dimensions the persistent ladder kernel would take the steps)
        for k in (0, 1, 2):
            kind = KIND_NAME[k]
            _add("sweep_lanes_kernel<%d, %d, false>" % (DP, k), cfg(D, Nt, 5 if (DP <= 128 and k == 1) else W, kind, **tk))
            _add("sweep_lanes_kernel<%d, %d, true>" % (DP, k), cfg(D, Nt, W, kind, **tk, **FEATURES[n % len(FEATURES)]))
            _add("sweep_lanes_ada_kernel<%d, %d>" % (DP, k), cfg(D, Nt, W, kind, ada=True, **tk, **(FEATURES[(n + 4) % len(FEATURES)] if n % 2 else {})))
            n += 1


def _mfma32_cases():
    """sweep_mfma32_kernel<KIND, HIST, MGEN, EV, compacted>: both matrix products of 32 dimensions on the matrix cores"""
    builds = (
        # hist, mgen, ev, compacted: what asks for it
        (False, 0, False, False, dict()),
        (True, 0, False, False, dict(hist=2)),
        (False, 0, True, False, dict(evolve=0.03)),
        (False, 0, False, True, dict()),
        (False, 0, True, True, dict(evolve=0.03)),
        (False, 1, False, False, dict(bounds="limit", oned=0.4)),
        (False, 1, True, False, dict(bounds="limit", mix=2, evolve=0.03)),
        (True, 1, False, False, dict(bounds="limit", hist=1)),                  # the box-bounds code with history, fixed ladder
        (True, 1, True, False, dict(bounds="limit", mean=True, hist=2, evolve=0.03)),
        (False, 1, False, True, dict(bounds="limit", mean=True)),
        (False, 1, True, True, dict(bounds="limit", oned=0.3, evolve=0.03)),
        (False, 2, False, False, dict(bounds="wrap", gauss_prior=True, oned=0.3)),
        (True, 2, False, False, dict(bounds="wrap", gauss_prior=True, hist=1, evolve=0.02)),   # the general state space with history
        (False, 3, False, True, dict(bounds="limit")),
        (False, 3, True, True, dict(bounds="limit", evolve=0.03)),
    )
    for k in (0, 2):
        for j, (hist, mgen, ev, comp, o) in enumerate(builds):
            kind = "diag" if (k == 2 and j % 4 == 1) else KIND_NAME[k]   # (a diagonal factor is a Cholesky factor to these kernels)
            Nt, W = (3, 1024) if comp else (5, 128 if (mgen, hist, ev) == (0, False, False) else 64)
            _add("sweep_mfma32_kernel<%d, %s, %d, %s, %s>" % (k, tf(hist), mgen, tf(ev), tf(comp)), cfg(29, Nt, W, kind, time_kernels=not comp, **o))


def _mfma_big_cases():
    """sweep_mfma64_kernel / sweep_mfma128_kernel<KIND, BND, EV>"""
    for DP in (64, 128):
        for k in (0, 2):
            for bnd in (False, True):
                for ev in (False, True):
                    o = {}
                    if bnd:
                        o["bounds"] = "limit"
                    if ev:
                        o["evolve"] = 0.03
                    kind = "diag" if (k == 2 and bnd and ev) else KIND_NAME[k]
                    _add("sweep_mfma%d_kernel<%d, %s, %s>" % (DP, k, tf(bnd), tf(ev)), cfg(dim_of(DP), 4, 128 if (k == 0 and bnd and not ev) else 64, kind, **o))


# the persistent ladder kernel's flavours (ladder_flavour in ptm_engine.hip) and what asks for each
FLAVOURS = {
    0: dict(),
    1: dict(oned=0.4),
    2: dict(hist=1),
    3: dict(mix=3, hist=2),
    4: dict(evolve=0.03),
    7: dict(oned=0.3, mix=2, hist=1, evolve=0.03),
    11: dict(de=True),
    15: dict(de=True, evolve=0.02),
    19: dict(bounds="wrap", gauss_prior=True),
    23: dict(bounds="wrap", gauss_prior=True, evolve=0.03, hist=1),
    27: dict(bounds="wrap", gauss_prior=True, de=True),
    31: dict(bounds="wrap", gauss_prior=True, de=True, evolve=0.02),
}


def _ladder_cases():
    """ladder_persistent_kernel<DP, KIND, FL> (a workgroup holds 256 / DP rungs) and ladder_steps_kernel<DP, KIND, T>"""
    n = 0
    for DP in (4, 8, 16, 32):
        D = dim_of(DP)
        for k in (0, 1):
            for fl, o in FLAVOURS.items():
                kind = "diag" if k else ("dense" if n % 2 else "lower")
                o = dict(o)
                if fl in (1, 2, 4, 19) and n % 3 == 0:
                    o["bounds"] = o.get("bounds", "limit")      # (open / limit boundaries are a run-time matter of the box builds)
                if fl in (0, 3) and n % 2:
                    o["mean"] = True
                # the builds with everything: ladders of two workgroups, the second ragged (3 rungs)
                # (the general state space without differential evolution accepts little beyond its coldest rungs: whole waves of walkers,
                #  so that Metropolis tests near their thresholds are met on every rung)
                Nt, W = (256 // DP + 3, 2) if fl in (7, 15, 31) else (6 if n % 2 else 5, 64 if fl in (19, 23) else 3)
                _add("ladder_persistent_kernel<%d, %d, %d>" % (DP, k, fl), cfg(D, Nt, W, kind, **o))
                n += 1
    for DP in (4, 8, 16):
        for k in (0, 1):
            for T in (64, 256):
                Nt = 4 if T == 64 else 64 // DP + 1
                _add("ladder_steps_kernel<%d, %d, %d>" % (DP, k, T), cfg(dim_of(DP), Nt, 1088, "diag" if k else ("lower" if T == 64 else "dense"),
                                                                       **(dict(oned=0.4) if T == 64 else dict(bounds="limit", hist=2))))


_sweep_kernel_cases()
_lanes_cases()
_mfma32_cases()
_mfma_big_cases()
_ladder_cases()

# Builds that no configuration accepted by both the engine and the checker (or tests/adaptive_model.py) reaches: name -> reason.
NOT_HELD = {}


def key(c):
    parts = ["D%d %dx%d %s" % (c["D"], c["Nt"], c["W"], c["kind"])]
    for k in sorted(c):
        if k in ("D", "Nt", "W", "kind") or not c[k]:
            continue
        parts.append(k if c[k] is True else "%s=%s" % (k, c[k]))
    return " ".join(parts)


def sweep_facts(c):
    """the SweepFacts of the configuration's PT step, as step_sweep_plan (ptm_engine.hip) fills them, in the order
    tests/cxx/census_plan_main.cc reads them; then the two environment bits"""
    kind = {"dense": 0, "diag": 1, "lower": 2}[c["kind"]]
    assert not c.get("de"), "no sweep case draws differential evolution (it is no template argument of a sweep kernel)"
    de, ada = False, bool(c.get("ada"))
    mix_K = c.get("mix") or 0
    return [padded(c["D"]), c["W"], c["Nt"] * c["W"], c["Nt"], kind,
            int(bool(c.get("bounds"))), int(c.get("bounds") == "limit"), int(not c.get("gauss_prior")), int(bool(c.get("mean"))), int(bool(c.get("oned"))),
            mix_K, int(bool(c.get("evolve"))), int(bool(c.get("hist")) or de), 0, 0, int(de), int(ada), 0, 1,
            int(c.get("env") == FORCE_VALU), 1]
