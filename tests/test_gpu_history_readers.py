"""The device's effective-sample-size and log-evidence kernels (ptm_ess_kernels.hpp, ptm_evidence_kernels.hpp) on history rings written
by every kernel that records history and in every row layout, against tests/ess_model.py / tests/evidence_model.py evaluated on the
engine's own history(), nhist and invtemps().  Bit for bit: NaN equals NaN, nwin / length / count exact -- sequential sums in the
host's order under -ffp-contract=off leave no tolerance to choose.

The rings, queries and seeds are those of tests/history_readers_util.py; tests/test_history_readers_cpu.py checks on the CPU
checker's copies of the same rings that the queries can tell a wrong row position from the right one."""
import numpy as np
import pytest

import history_readers_util as U

pytestmark = pytest.mark.gpu


def stepped(ring, eng, steps=None):
    """the named kernel is the writer; step() returns with the persistent ladder kernel's launch still pending"""
    assert eng.step_kernel_name == ring.writer and eng.sweep_kernel_name == ring.sweep, (ring.name, eng.step_kernel_name, eng.sweep_kernel_name)
    eng.step(steps or ring.steps)
    return eng


def settled(ring, eng):
    """(history, nhist, invtemps) once everything is committed; the persistent ladder kernel has not given up"""
    eng.sync()
    if ring is not None and ring.writer.startswith("ladder_persistent_kernel"):
        st = eng.ladder_stats()
        assert st["launches"] >= 1 and st["fallbacks"] == 0 and not st["disabled"], st
    return eng.history(), eng.nhist, eng.invtemps()


# ---- effective sample size ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ess_rings():
    """name -> (engine, history, nhist, what the first call gave): built once, read by every case of the ring"""
    made = {}

    def get(name):
        if name not in made:
            ring = U.RINGS[name]
            eng = stepped(ring, U.ring_engine(ring))
            first = None
            if ring.pending:      # no sync() between step() and the first estimator call: the launch is still pending
                first = eng.ess_windowed(1, ring.D, *ring.shapes[0])
                assert eng.ess_last_on_device
            hist, nhist, _ = settled(ring, eng)
            assert eng.nsize.max() <= ring.cap                           # the ring holds the whole run
            nh = nhist.reshape(ring.Nt, ring.W)
            assert (nh >= ring.steps).all() and len(set(nh[1].tolist())) > 1, nh[1]   # walkers of a rung differ in their counts
            made[name] = (eng, hist, nhist, first)
        return made[name]
    yield get
    for eng, _, _, _ in made.values():
        eng.close()


ESS_CASES = [(r.name, rung, k) for r in U.RINGS.values() for rung in U.ess_rungs(r) for k in range(len(r.shapes))]


@pytest.mark.parametrize("name,rung,k", ESS_CASES, ids=["%s-rung%d-%dx%d" % (n, r, U.RINGS[n].shapes[k][0], U.RINGS[n].shapes[k][1]) for n, r, k in ESS_CASES])
def test_ess_on_the_ring_of_every_recording_kernel(ess_rings, name, rung, k):
    ring = U.RINGS[name]
    eng, hist, nhist, first = ess_rings(name)
    width, every, burn = ring.shapes[k]
    model = U.EssModel(hist, nhist, ring.W, rung, ring.add, ring.D)
    for nfeat in U.nfeats(ring):
        w_ess, w_nwin = model.windowed(nfeat, width, every, burn)
        assert (w_nwin > 0).all()
        ess, nwin = eng.ess_windowed(rung, nfeat, width, every, burn)
        assert eng.ess_last_on_device
        bad = np.flatnonzero((ess.view(np.uint64) != w_ess.view(np.uint64)) | (nwin != w_nwin))
        assert len(bad) == 0, (name, rung, nfeat, ring.shapes[k], bad[:4], ess[bad[:4]], w_ess[bad[:4]], nwin[bad[:4]], w_nwin[bad[:4]])
        r_ess, r_len = model.report(nfeat, width, every)
        ess, length = eng.effective_samples(rung, nfeat, width, every, -1)
        assert eng.ess_last_on_device
        bad = np.flatnonzero((ess.view(np.uint64) != r_ess.view(np.uint64)) | (length != r_len))
        assert len(bad) == 0, (name, rung, nfeat, ring.shapes[k], "report", bad[:4], ess[bad[:4]], r_ess[bad[:4]], length[bad[:4]], r_len[bad[:4]])
    if first is not None and rung == 1 and k == 0:       # the call that found the launch pending
        w_ess, w_nwin = model.windowed(ring.D, width, every, burn)
        assert U.same_bits(first[0], w_ess) and np.array_equal(first[1], w_nwin), (name, first[0][:4], w_ess[:4])


# ---- log-evidence ------------------------------------------------------------------------------------------------------------------
def check_evidence(eng, got, ilen, add, what):
    hist, nhist, beta = eng.history(), eng.nhist, eng.invtemps()
    want = U.evidence_model(hist, nhist, beta, eng.Nt, eng.W, ilen, add)
    U.assert_evidence(got, want, what)
    return got, nhist


@pytest.mark.parametrize("name", U.EVIDENCE_RINGS)
def test_evidence_on_the_ring_of_every_recording_kernel(name):
    """ring A: more than 256 walkers (several workgroups of the totals' kernel, r = c / W across workgroups), every rung recorded in a
    short ring that has wrapped; B and F: the call follows step() with the persistent ladder kernel's launch still pending"""
    ring = U.RINGS[name]
    eng = U.ring_engine(ring, history_rungs=ring.Nt, cap=U.A_EVIDENCE_CAP if name == "A" else ring.cap)
    try:
        stepped(ring, eng)
        if not ring.pending:
            eng.sync()
        got = eng.log_evidence(ring.ilen)
        settled(ring, eng)
        (ev, up, down, count), nhist = check_evidence(eng, got, ring.ilen, ring.add, name)
        assert np.isfinite(ev).all() and (count > 0).all()
        assert len(set(nhist.reshape(ring.Nt, ring.W)[1].tolist())) > 1
        assert ring.ilen % ring.add or ring.add == 1
        if name == "A":
            assert ring.W > 256 and eng.nsize.min() > eng.hist_cap          # wrapped
    finally:
        eng.close()


def test_evidence_with_every_edge_at_once():
    """a wrapped ring, add_every_n = 3, evolving ladders and walkers with different add_state counts, ilen no multiple of 3, windows
    that are no multiple of the 8 rows loaded ahead"""
    c = U.EDGES
    eng = U.make_engine(c["D"], c["Nt"], c["W"], "lower", c["add"], c["seed"], c["swap_rate"], c["Nt"], c["cap"], evolve=c["evolve"])
    try:
        eng.step(c["steps"])
        eng.sync()
        (ev, up, down, count), nhist = check_evidence(eng, eng.log_evidence(c["ilen"]), c["ilen"], c["add"], "edges")
        beta = eng.invtemps()
        assert eng.nsize.min() > c["cap"] and c["ilen"] % c["add"] and len(set(nhist.tolist())) > 3
        assert not np.array_equal(beta[0], beta[1])
        assert np.isfinite(ev).all() and (count > 0).all() and (count % 8 != 0).all() and len(set(count.ravel().tolist())) > 1
    finally:
        eng.close()


def test_ilen_swept_across_the_chains_own_counts():
    """chains with nhist < ilen have an empty window: count 0 and NaN; their neighbours' ratios follow the model"""
    s = U.SWEEP
    eng = U.make_engine(s["D"], s["Nt"], s["W"], "lower", s["add"], s["seed"], s["swap_rate"], s["Nt"], s["cap"])
    try:
        eng.step(s["steps"])
        eng.sync()
        nhist = eng.nhist
        nh = nhist.reshape(s["Nt"], s["W"])
        mixed = 0
        for ilen in U.sweep_ilens(nhist):
            (ev, up, down, count), _ = check_evidence(eng, eng.log_evidence(ilen), ilen, s["add"], "ilen %d" % ilen)
            empty = nh < ilen
            assert np.array_equal(count == 0, empty)
            assert np.array_equal(np.isnan(up), empty[1:]) and np.array_equal(np.isnan(down), empty[:-1])
            assert np.array_equal(np.isnan(ev), empty.any(axis=0))
            mixed += bool(empty.any() and not empty.all())
        assert mixed >= 1
    finally:
        eng.close()


# ---- checkpoint and resume ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["B", "F"])
def test_estimators_after_checkpoint_and_resume(name):
    """a fresh engine restored from a checkpoint and stepped on gives the uninterrupted engine's ESS and evidence bit for bit"""
    ring = U.RINGS[name]
    half = ring.steps // 2
    a, b = U.ring_engine(ring), U.ring_engine(ring)
    try:
        stepped(ring, a, half)
        ck = a.checkpoint()
        b.restore(ck)
        stepped(ring, a, ring.steps - half)
        stepped(ring, b, ring.steps - half)
        out = []
        for eng in (a, b):        # (the first call of each finds its launch pending)
            o = [eng.log_evidence(ring.ilen)]
            for rung in U.ess_rungs(ring):
                for shape in ring.shapes:
                    for nfeat in (ring.D, 5):
                        o += [eng.ess_windowed(rung, nfeat, *shape), eng.effective_samples(rung, nfeat, shape[0], shape[1], -1)]
                        assert eng.ess_last_on_device
            out.append(o)
            settled(ring, eng)
        for x, y in zip(*out):
            assert len(x) == len(y) and all(U.same_bits(p, q) if p.dtype.kind == "f" else np.array_equal(p, q) for p, q in zip(x, y))
        assert np.array_equal(a.nhist, b.nhist)
        check_evidence(b, out[1][0], ring.ilen, ring.add, name + " resumed")
        model = U.EssModel(b.history(), b.nhist, ring.W, 1, ring.add, ring.D)
        w_ess, w_nwin = model.windowed(ring.D, *ring.shapes[0])
        k = 1 + 4 * (U.ess_rungs(ring).index(1) * len(ring.shapes))
        assert U.same_bits(out[1][k][0], w_ess) and np.array_equal(out[1][k][1], w_nwin) and (w_nwin > 0).all()
    finally:
        a.close(); b.close()
