"""The rings of tests/test_gpu_history_readers.py and tests/test_history_readers_cpu.py: one shape per kernel that records history and
per row layout, the queries the estimators are asked on each, the models' answers on a history()-shaped ring, and the same rings from
the CPU checker (its ring is the engine's bit for bit: test_history_rows_match_the_oracle), so that what the GPU tests rely on -- the
queries can tell a wrong row position from the right one -- is checked without a GPU.

A ring is the dict Engine.history() returns (x [cap][chains][D], llike, row [cap][chains]; chain = rung * W + walker), `nhist` the
chains' add_state counts and `beta` [W][Nt] the walkers' inverse temperatures."""
import collections

import numpy as np

import ess_model as EM
import evidence_model as VM

Ring = collections.namedtuple("Ring", "name D Nt W kind add steps hist_rungs cap writer sweep permuted pending shapes ilen seed swap_rate")
# shapes: (width, every, burn) -- every a multiple of add_every_n (rows linear in the sample number), every not a multiple (a
# division per sample; on ring A, add_every_n = 1, there is no such stride), and span = (width // every) * every < width.
# cap: the ring holds the whole run (1 + ceil(max nhist / add_every_n) rows; the CPU file checks that it does).
RINGS = collections.OrderedDict((r.name, r) for r in (
    Ring("A", 21, 4, 320, "lower", 1, 520, 2, 600, "decide_kernel + sweep_mfma32_kernel<2, true, 0, false, false>", "sweep_mfma32_kernel<2, true, 0, false, false>",
         True, False, ((100, 1, 2), (104, 4, 2), (100, 3, 2)), 150, 0x5EED0A01, 0.3),
    Ring("B", 20, 7, 3, "dense", 2, 800, 7, 600, "ladder_persistent_kernel<32, 0, 2>", "sweep_lanes_kernel<32, 0, false>",
         True, True, ((150, 2, 2), (150, 3, 2), (155, 4, 2)), 301, 0x5EED0B02, 0.4),
    Ring("C", 40, 5, 3, "dense", 2, 800, 5, 600, "decide_kernel + sweep_lanes_kernel<64, 0, false>", "sweep_lanes_kernel<64, 0, false>",
         True, False, ((150, 2, 2), (150, 3, 2), (155, 4, 2)), 301, 0x5EED0C03, 0.4),
    Ring("D", 100, 4, 3, "lower", 2, 700, 4, 500, "decide_kernel + sweep_lanes_kernel<128, 2, false>", "sweep_lanes_kernel<128, 2, false>",
         True, False, ((130, 2, 2), (130, 5, 2), (135, 4, 2)), 0, 0x5EED0D04, 0.4),
    Ring("E", 150, 4, 2, "lower", 2, 700, 4, 500, "decide_kernel + sweep_lanes_kernel<256, 2, false>", "sweep_lanes_kernel<256, 2, false>",
         False, False, ((130, 2, 2), (130, 5, 2), (135, 4, 2)), 0, 0x5EED0E05, 0.4),
    Ring("F", 12, 24, 5, "diag", 3, 1200, 24, 600, "ladder_persistent_kernel<16, 1, 2>", "sweep_lanes_kernel<16, 1, false>",
         False, True, ((200, 3, 2), (200, 2, 2), (205, 6, 2)), 401, 0x5EED0F06, 0.3),
))
EVIDENCE_RINGS = ("A", "B", "C", "F")
A_EVIDENCE_CAP = RINGS["A"].ilen + 2          # ring A's evidence engine records every rung in a short ring: wrapped
# the combined-edges evidence case: wrapped ring, add_every_n = 3, evolving ladders, walkers with different nhist; ilen no multiple
# of 3 and a window (ilen // 3 rows or one more) that is no multiple of the 8 rows the kernel loads ahead
EDGES = dict(D=2, Nt=6, W=70, add=3, steps=500, ilen=200, cap=75, evolve=0.01, seed=0xE71D5, swap_rate=0.4)
# ilen swept across the chains' own counts
SWEEP = dict(D=2, Nt=5, W=70, add=1, steps=200, cap=404, seed=0xE71D6, swap_rate=0.4)


def nfeats(ring):
    """every nfeat in 1 .. min(D, 12) -- they cut inside and across the 8-double blocks of the permutation -- and D"""
    return list(range(1, min(ring.D, 12) + 1)) + [ring.D]


def ess_rungs(ring):
    """rung 0, the last recorded rung, and rung 1: the coldest and the hottest rung have one neighbour and are never exchanged twice
    in a step, a rung between them is, and its walkers differ in their add_state counts"""
    return sorted({0, 1, ring.hist_rungs - 1})


def row_pos(f):
    """where feature f of a 32-, 64- or 128-dimension padded row is stored (the kernels' row_pos)"""
    return 8 * (f >> 3) + 2 * (f & 3) + ((f >> 2) & 1)


def same_bits(a, b):
    """the same doubles bit for bit, NaN equal to NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def sweep_ilens(nhist):
    lo, hi = int(np.min(nhist)), int(np.max(nhist))
    return [lo - 1, lo, lo + 1, hi, hi + 1]


# ---- engines -----------------------------------------------------------------------------------------------------------------
def problem(D, Nt):
    import parity_util as PU
    return PU.problem_for(D, Nt, 1e2)


def make_engine(D, Nt, W, kind, add, seed, swap_rate, history_rungs, cap, evolve=0.0):
    """an engine on the synthetic Gaussian problem, at its first draw from the prior, not stepped"""
    from ptmcmc_amd import engine as E
    eng = E.Engine(D, Nt, W, seed=seed, swap_rate=swap_rate, add_every_n=add, history_rungs=history_rungs, history_capacity=cap)
    problem(D, Nt).configure(eng, {"lower": E.PROP_LOWER, "dense": E.PROP_DENSE, "diag": E.PROP_DIAG}[kind])
    if evolve > 0:
        eng.set_evolve_temps(evolve)
    eng.init_from_prior()
    return eng


def ring_engine(ring, history_rungs=None, cap=None):
    return make_engine(ring.D, ring.Nt, ring.W, ring.kind, ring.add, ring.seed, ring.swap_rate, history_rungs or ring.hist_rungs, cap or ring.cap)


# ---- the models on a ring ---------------------------------------------------------------------------------------------------
class _Features(EM.Estimator):
    """the estimator of a group of series for every nfeat at once: a feature is a lane of its own, so the per-feature numbers of all
    D features answer each nfeat <= D (Estimator.windowed takes the minimum over the first nfeat of them)"""

    def __init__(self, steps, nseries, dim, reader):
        EM.Estimator.__init__(self, steps, nseries, dim, reader)
        self.all, self.cache = EM.Estimator(steps, nseries, dim, reader), {}

    def feature_ess(self, width, every, burn):
        key = (width, every, burn)
        if key not in self.cache:
            self.cache[key] = self.all.feature_ess(width, every, burn)
        return self.cache[key]


class EssModel:
    """tests/ess_model.py on local rung `rung` of a ring: the walkers are grouped by their add_state counts (a series' windows follow
    from its own length), every walker's answer is the model's for its own count.  stored_order=True reads feature f from position
    f of the stored row: what the device would do with the identity in place of row_pos."""

    def __init__(self, hist, nhist, W, rung, add, dim, stored_order=False):
        self.W, self.dim = W, dim
        counts = np.asarray(nhist).reshape(-1, W)[rung]
        if stored_order:
            dp = 32 if dim <= 32 else 64 if dim <= 64 else 128
            inv = {row_pos(f): f for f in range(dp)}
            x = hist["x"]
            wrong = np.zeros_like(x)                      # (a position that holds a padding lane reads 0)
            for f in range(dim):
                if inv[f] < dim:
                    wrong[:, :, f] = x[:, :, inv[f]]
            hist = dict(hist, x=wrong)
        self.groups = []
        for c in sorted(set(counts.tolist())):
            who = np.flatnonzero(counts == c)
            self.groups.append((who, _Features(c, len(who), dim, EM.ring_reader(hist, rung * W + who, add))))

    def _gather(self, call, dtype):
        a, b = np.zeros(self.W), np.zeros(self.W, dtype=dtype)
        for who, est in self.groups:
            a[who], b[who] = call(est)
        return a, b

    def windowed(self, nfeat, width, every, burn):
        def call(est):
            est.nfeat = nfeat
            return est.windowed(width, every, burn)
        return self._gather(call, np.int32)

    def report(self, nfeat, width, every):
        def call(est):
            est.nfeat = nfeat
            return est.report(width, every, -1)
        return self._gather(call, np.int32)


def evidence_model(hist, nhist, beta, Nt, W, ilen, add):
    """tests/evidence_model.py for every walker's ladder: (log_evidence [W], up, down [Nt - 1][W], count [Nt][W])"""
    ev, up, down, count = np.empty(W), np.empty((Nt - 1, W)), np.empty((Nt - 1, W)), np.empty((Nt, W), dtype=np.int32)
    ll, row = hist["llike"], hist["row"]
    for w in range(W):
        ev[w], up[:, w], down[:, w], count[:, w] = VM.ring_total(ll, row, nhist, beta[w], Nt, W, w, ilen, add)
    return ev, up, down, count


def assert_evidence(got, want, what=""):
    for name, g, m in zip(("log_evidence", "up", "down"), got[:3], want[:3]):
        bad = np.argwhere(~((g.view(np.uint64) == m.view(np.uint64)) | (np.isnan(g) & np.isnan(m))))
        assert len(bad) == 0, (what, name, bad[:4].tolist(), g[tuple(bad[0])], m[tuple(bad[0])])
    assert np.array_equal(got[3], want[3]), (what, "count", np.argwhere(got[3] != want[3])[:4].tolist())


# ---- the same rings from the CPU checker ------------------------------------------------------------------------------------------
def oracle_ring(D, Nt, W, kind, add, seed, swap_rate, steps, rungs, evolve=0.0):
    """(ring, nhist, beta) of the first `rungs` rungs as the engine would hold them in a ring that keeps the whole run, from
    oracle_lib.Ladder; the start states are the checker's own first draw from the prior (the engine's: test_init_from_prior_matches_oracle)"""
    import oracle_lib as O
    import parity_util as PU
    from ptmcmc_amd import engine as E
    pr = problem(D, Nt)
    ekind = {"lower": E.PROP_LOWER, "dense": E.PROP_DENSE, "diag": E.PROP_DIAG}[kind]
    fac = pr.proposal_factors(range(Nt), lower=(kind != "dense"))
    if kind == "diag":
        fac = np.stack([np.sqrt(np.diag(T @ T.T)) for T in fac])
    lad = O.Ladder(PU.oracle_problem(pr), pr.beta, W=W, swap_rate=swap_rate, add_every_N=add)
    lad.set_proposals([(PU.KIND_TO_ORACLE[ekind], fac[r], 0.0) for r in range(Nt)])
    lad.use_philox(seed)
    cap = 2 + (steps + steps // 2) // add                # (the checker drops what does not fit: checked below)
    lad.enable_history(cap)
    lad.init_from_prior(seed)
    if evolve > 0:
        lad.evolve_temps(evolve)
    lad.pt_step(steps)
    nsize, nhist = PU.to_engine_order(lad.nsize, Nt, W), PU.to_engine_order(lad.nhist, Nt, W)
    assert nsize.max() <= cap
    h = lad.history()
    keep = rungs * W

    def engine_shape(a):       # [N][cap](, D) in the checker's chain order -> [cap][chains](, D) in the engine's
        a = a.reshape((W, Nt, cap) + a.shape[2:])
        return np.ascontiguousarray(np.moveaxis(a, 2, 0).swapaxes(1, 2).reshape((cap, Nt * W) + a.shape[3:])[:, :keep])
    row = np.where(np.arange(cap)[:, None] < nsize[None, :keep], np.arange(cap, dtype=np.int32)[:, None], -1).astype(np.int32)
    ring = dict(x=engine_shape(h["x"]), llike=engine_shape(h["llike"]), row=row)
    return ring, nhist, lad.betaw, nsize


def wrapped(ring, nsize, cap):
    """what a ring of `cap` slots still holds of a ring that kept everything: saved row s sits in slot s % cap, the newest one wins"""
    chains = ring["row"].shape[1]
    out = dict(x=np.zeros((cap, chains) + ring["x"].shape[2:]), llike=np.zeros((cap, chains)), row=np.full((cap, chains), -1, dtype=np.int32))
    for c in range(chains):
        rows = np.arange(max(0, int(nsize[c]) - cap), int(nsize[c]))
        for k in ("x", "llike", "row"):
            out[k][rows % cap, c] = ring[k][rows, c]
    return out


def oracle_of(ring, rungs=None):
    return oracle_ring(ring.D, ring.Nt, ring.W, ring.kind, ring.add, ring.seed, ring.swap_rate, ring.steps, rungs or ring.hist_rungs)
