"""One run of a big-population engine against the CPU oracle in a process of its own (PTM_BOX_PREFILTER is read once per process):
the box pre-pass (ptmcmc_amd/csrc/ptm_box_prefilter.hpp) must change nothing in the chains.  Prints the pre-pass's counters.
usage: python box_prefilter_worker.py lower|dense|nonfinite|sharded|sharded_overlap|aged   (aged: `lower` late in a run, tests/aging_util.py)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ptmcmc_amd import engine as E
import parity_util as PU

D, NT, W, SR = 32, 12, 1024, 0.3


class DevShard:
    """EngineShard with raw device buffers instead of torch tensors (the five methods shard_sim uses)."""

    def __init__(self, eng):
        self.e = eng
        self.W, self.nloc, self.r0, self.Nt = eng.W, eng.nloc, eng.r0, eng.Nt
        self.row_doubles = eng.exchange_buffer_doubles

    def alloc(self, n):
        return E.DeviceBuffer(n * 8)

    def copy_llike(self, first, n, dst):
        self.e.copy_llike(first, n, dst.ptr)

    def exchange_decide(self, lb, la, halo, su, sd):
        p = lambda b: None if b is None else b.ptr
        self.e.exchange_decide(p(lb), p(la), halo, p(su), p(sd))

    def finish_and_sweep(self, rb, ra):
        p = lambda b: None if b is None else b.ptr
        self.e.exchange_finish_and_sweep(p(rb), p(ra))

    def install(self, rb, ra):
        p = lambda b: None if b is None else b.ptr
        self.e.exchange_install(p(rb), p(ra))

    def sweep_rungs(self, first, n, closes_step):
        self.e.sweep_rungs(first, n, closes_step)

    can_overlap = True
    gathered = False
    needs_lprior = False

    def sync(self):
        self.e.sync()

    @staticmethod
    def sub(buf, off, n):
        return buf.slice(off * 8, n * 8)

    def dcopy(self, dst, src):
        self.e.sync()
        dst.copy_from(src.ptr, min(dst.nbytes, src.nbytes))


def counts(engines):
    tot = dict(seen=0, settled=0, rungs_flagged=0, eligible=1, rungs=0)
    for e in engines:
        # (a library from before the pre-pass, PTM_ENGINE_LIB: the same run with nothing to count)
        c = e.prefilter_counts() if hasattr(e.L, "ptm_get_prefilter_counts") else dict(seen=0, settled=0, rungs_flagged=0, eligible=0)
        tot["seen"] += c["seen"]; tot["settled"] += c["settled"]; tot["rungs_flagged"] += c["rungs_flagged"]
        tot["eligible"] &= int(c["eligible"]); tot["rungs"] += e.nloc
    return "seen=%(seen)d settled=%(settled)d rungs_flagged=%(rungs_flagged)d rungs=%(rungs)d eligible=%(eligible)d" % tot


def run_pair(kind, x0=None, aged=False):
    """3 + 4 + 5 PT steps, plain sweeps and a checkpoint / resume in between; engine and oracle bit for bit after each leg.
    aged: after the first leg engine and oracle are put at PT step 2^32 - 2 with every counter shifted up to 16 below PTM_COUNT_MAX
    at the run's end -- the next leg's steps cross 2^32, the labels are in use and the compacted sweeps leave their one add per chain
    to the engine's count (nhist_flush_kernel) up there."""
    pr, eng, lad = PU.make_pair(D, NT, W, 1e9, kind=kind, swap_rate=SR, x0=x0)
    assert eng.sweep_kernel_name.endswith(", 0, false, true>"), eng.sweep_kernel_name
    eng.step(3); eng.sync(); lad.pt_step(3)
    PU.assert_same_state(eng, lad, "after 3 steps")       # (eng.states() puts labelled rows back: restore_rows_kernel)
    shift = 0
    same = PU.assert_same_state
    if aged:
        import aging_util as AU
        view, shift = AU.age_pair(eng, lad, 2 + 4 + 5)
        assert eng.step_count == lad.step == AU.LATE_STEP and eng.sweep_kernel_name.endswith(", 0, false, true>")
        same = lambda e, l, what: PU.assert_same_state(AU.AgedView(e, shift), l, what)     # (add_every_n = 1: the row counts are shifted alike)
        same(eng, lad, "aged")
        eng.step(3); eng.sync(); lad.pt_step(3)
        assert (eng.row_labels != np.repeat(np.arange(NT, dtype=np.int32), W)).any(), "the labelled path did not run"
        assert eng.step_count == 2**32 + 1
        same(eng, lad, "aged, after the 3 steps across 2^32")
        t, a = eng.counter_sums()
        assert (t, a) == (int(eng.ntries.astype(np.int64).sum()), int(eng.naccept.astype(np.int64).sum()))
    eng.sweep(2); eng.sync(); lad.sweep(2)
    same(eng, lad, "after plain sweeps")
    eng.step(1 if aged else 4); lad.pt_step(1 if aged else 4)
    ck = eng.checkpoint()
    same(eng, lad, "after 7 steps")
    e2 = E.Engine(D, NT, W, swap_rate=SR)
    pr.configure(e2, kind)
    e2.restore(ck)
    for e in (eng, e2):
        e.step(5); e.sync()
    lad.pt_step(5)
    same(eng, lad, "after 12 steps")
    same(e2, lad, "resumed engine after 12 steps")
    t, a = eng.swap_counts()
    assert np.array_equal(t, lad.swap_count) and np.array_equal(a, lad.swap_accept_count)
    acc = int(eng.naccept.astype(np.int64).sum() - eng.Nc * (1 + shift))
    if aged:
        import aging_util as AU
        top = int(max(eng.ntries.max(), eng.nhist.max()))
        assert AU.COUNT_MAX - AU.MARGIN - 2 * 11 <= top <= AU.COUNT_MAX - AU.MARGIN, top
    out = counts([eng]) + " accepts=%d" % acc
    eng.close(); e2.close()
    return out


def run_nonfinite():
    """a few hundred chains start outside the prior box (lprior -inf): their log-Hastings ratio is NaN and the move is accepted wherever
    the proposal lands, so the pre-pass must hand them to the sweep whatever its box test says"""
    pr = PU.problem_for(D, NT, 1e9)
    rng = np.random.default_rng(2024)
    c, h = np.asarray(pr.centers, float), np.asarray(pr.halfwidths, float)
    x0 = c + h * rng.uniform(-1.0, 1.0, size=(NT * W, D))
    rows = rng.choice(NT * W, size=300, replace=False)
    dims = rng.integers(0, D, size=300)
    x0[rows, dims] = c[dims] + h[dims] * rng.choice([-1.5, 1.5], size=300)
    inside = np.all(np.abs(x0 - c) <= h, axis=1)
    return run_pair(E.PROP_LOWER, x0=x0) + " outside=%d outside_rungs=%d" % (int((~inside).sum()), len(set((np.flatnonzero(~inside) // W).tolist())))


def run_sharded(overlap):
    """the body of test_compacted_sweep_in_sharded_engines: partial sweeps (interior / boundary rungs separately) of rung shards"""
    import shard_sim
    from ptmcmc_amd.parallel import shard_bounds
    from ptmcmc_amd.problems import GaussianProblem
    Nt, G = 24, 3
    pr = GaussianProblem(D, Nt, 1e3)
    ref = E.Engine(D, Nt, W, swap_rate=SR)
    pr.configure(ref, E.PROP_LOWER)
    ref.init_from_prior()
    x0 = ref.states()
    shards = []
    for g in range(G):
        r0, n = shard_bounds(Nt, G, g)
        e = E.Engine(D, Nt, W, swap_rate=SR, rung_begin=r0, rung_count=n)
        pr.configure(e, E.PROP_LOWER)
        e.set_states(x0[r0 * W:(r0 + n) * W])
        shards.append(e)
    lads = shard_sim.build([DevShard(e) for e in shards], halo=4)
    copy = lambda dst, src: dst.copy_from(src.ptr)
    for k in range(3):
        ref.step(4)
        (shard_sim.step_overlapped if overlap else shard_sim.step)(lads, copy, 4)
        assert np.array_equal(np.concatenate([e.states() for e in shards]), ref.states()), "states differ after step %d" % (4 * k + 4)
    for name in ("llike", "ntries", "naccept", "nhist", "last_type"):
        assert np.array_equal(np.concatenate([getattr(e, name) for e in shards]), getattr(ref, name)), name
    out = counts(shards)
    for e in shards + [ref]:
        e.close()
    return out


if __name__ == "__main__":
    case = sys.argv[1]
    if case == "lower":
        res = run_pair(E.PROP_LOWER)
    elif case == "aged":
        res = run_pair(E.PROP_LOWER, aged=True)
    elif case == "dense":
        res = run_pair(E.PROP_DENSE)
    elif case == "nonfinite":
        res = run_nonfinite()
    elif case in ("sharded", "sharded_overlap"):
        res = run_sharded(case == "sharded_overlap")
    else:
        raise SystemExit("unknown case " + case)
    print("ok " + res)
