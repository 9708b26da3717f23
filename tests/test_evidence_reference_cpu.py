"""The log-evidence estimators against the real reference's own answers (tests/golden/evidence.json.gz, recorded by
oracle/ref_driver.cc golden-evidence from parallel_tempering_chains::log_evidence_ratio, bestEvidenceErr and what a do_evid ladder
prints): tests/evidence_model.py and the facade's evidence_estimator / evidence_records (through tests/cxx/evidence_fixture_main.cc)
must give every recorded answer bit for bit and every printed line string for string, and the fixture must be able to tell the right
reading of chain.cc from each of the named wrong ones (tests/evidence_reference_util.py)."""
import math

import pytest

import evidence_model as M
import evidence_reference_util as U
from test_evidence_cpu import fixture_exe, run   # noqa: F401  (the compiled fixture program, one per module)


def short_ladders():
    return [(g, k, lad) for g in U.load()["groups"] for k, lad in enumerate(g["ladders"])]


def test_the_fixture_has_the_groups_and_the_edges_the_comparison_needs():
    fx = U.load()
    assert [g["name"] for g in fx["groups"]] == ["A", "D", "B", "C"]
    want = {"A": (4, 1, 1, False), "B": (3, 3, 5, False), "C": (2, None, None, False), "D": (4, 3, None, True)}
    for g in fx["groups"]:
        nt, a, ninit, evolving = want[g["name"]]
        assert g["Nt"] == nt and (a is None or g["add_every_N"] == a) and (ninit is None or g["Ninit"] == ninit) and (g["evolve_rate"] > 0) == evolving
        assert len(g["ladders"]) >= 4
        assert len({tuple(lad["Nhist"]) for lad in g["ladders"]}) == len(g["ladders"])              # Nhist differs between the walkers-to-be
        for lad in g["ladders"]:
            assert all(len(rows) == n for rows, n in zip(lad["llike"], lad["Nsize"]))
            assert all(n == g["Ninit"] + (h - 1) // g["add_every_N"] + 1 for n, h in zip(lad["Nsize"], lad["Nhist"]))   # chain.hh: getStep = Nhist, size = Nsize
            assert all(len(set(rows[-30:])) > 5 for rows in lad["llike"])                            # no constant series
            lo, hi = min(lad["Nhist"]), max(lad["Nhist"])
            assert [q["ilen"] for q in lad["queries"]] == [1, 2, 3, 4, 7, 50, lo - 1, lo, lo + 1, hi, hi + 1, 10**6]
            flat = [U.num(v) for q in lad["queries"] for v in q["ab"]]
            assert any(math.isnan(v) for v in flat) and any(math.isfinite(v) for v in flat)
            assert all(math.isnan(U.num(v)) for v in lad["queries"][0]["ab"])                        # ilen = 1: an empty window
        if g["Nt"] > 2:   # a rung exchanged twice in a step has one more add_state call: the chains of a ladder differ,
            mixed = [q for lad in g["ladders"] for q in lad["queries"] if any(math.isnan(U.num(v)) for v in q["ab"]) and any(math.isfinite(U.num(v)) for v in q["ab"])]
            assert mixed                                                                             # ... so one call has NaN and finite answers
    d = U.group("D")
    assert all(lad["invtemp"] != lad["invtemp0"] and lad["invtemp"][0] == 1 for lad in d["ladders"])
    assert all(lad["invtemp"] == lad["invtemp0"] for name in "ABC" for lad in U.group(name)["ladders"])
    assert [lad["verbose"] for lad in fx["long"]] == [1, 0]
    for lad in fx["long"]:
        assert lad["Nt"] == 3 and lad["add_every_N"] == 10 and lad["bin"] == 20000 and len(lad["reports"]) == 8
        assert [r["step"] for r in lad["reports"]] == [20000 * k for k in range(1, 9)]
        assert len(set(lad["Nhist"])) > 1
        assert any(line.startswith("0: N=") for line in lad["reports"][5]["lines"])                  # the sixth report has the first standard error
        assert any(line.startswith("i=2 ") for line in lad["reports"][7]["lines"])                   # the second pyramid level


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_the_model_gives_every_recorded_ratio_bit_for_bit(name):
    g = U.group(name)
    for k, lad in enumerate(g["ladders"]):
        for q in lad["queries"]:
            rec = [U.num(v) for v in q["ab"]]
            got = U.pair_answers(g, lad, q["ilen"])
            assert len(got) == len(rec) == 2 * (g["Nt"] - 1)
            assert all(U.same_bits(r, c) for r, c in zip(rec, got)), (name, k, q["ilen"], rec, got)
            ev, up, down, count = U.model_total(g, lad, q["ilen"])                                   # the total's up / down are those ratios
            assert all(U.same_bits(up[i], rec[2 * i]) and U.same_bits(down[i], -rec[2 * i + 1]) for i in range(g["Nt"] - 1))
            assert math.isnan(ev) == any(math.isnan(v) for v in rec)
            assert all((c == 0) == (q["ilen"] > h or q["ilen"] == 1 or (h - q["ilen"]) // g["add_every_N"] == (h - 1) // g["add_every_N"])
                       for c, h in zip(count, lad["Nhist"]))


@pytest.mark.parametrize("verbose", [1, 0])
def test_the_model_gives_the_long_ladders_ratios_totals_lines_and_best_stderr(verbose):
    lad = next(l for l in U.load()["long"] if l["verbose"] == verbose)
    rec = M.Records()
    for k, rep in enumerate(lad["reports"]):
        want = [U.num(v) for v in rep["query"]["ab"]]
        got = U.pair_answers(lad, lad, lad["bin"], snap=rep)
        assert all(math.isfinite(v) for v in want)
        assert all(U.same_bits(r, c) for r, c in zip(want, got)), (k, want, got)
        ev, up, down, count = U.model_total(lad, lad, lad["bin"], snap=rep)
        assert all(1998 <= c <= 2000 for c in count), count
        assert rep["lines"][0] == "Total log-evidence: " + M.g(ev)
        assert rec.push(ev, bool(verbose)) == rep["lines"], (k, rep["lines"])
        assert U.same_bits(rec.best, U.num(rep["best"])), (k, rec.best, rep["best"])
    assert rec.best < 1e100 and len(rec.records) == 3


def ladder_words(g, lad, ilen, snap=None):
    snap = snap or lad
    words = ["ladder_init", g["Ninit"], g["Nt"], 1, g["add_every_N"], ilen]
    for r in range(g["Nt"]):
        rows = lad["llike"][r][:snap["Nsize"][r]]
        words += [snap["Nhist"][r], len(rows)] + [repr(v) for v in rows]
    return words + [repr(U.num(b)) for b in snap["invtemp"]]


def parse(line):
    return [[float(x) for x in part.split()] for part in line[2:].split("|")]


def test_the_facades_estimator_gives_every_recorded_ratio_bit_for_bit(fixture_exe):
    jobs = [(g, lad, q["ilen"], None, q["ab"]) for g, _, lad in short_ladders() for q in lad["queries"]]
    jobs += [(lad, lad, lad["bin"], rep, rep["query"]["ab"]) for lad in U.load()["long"] for rep in lad["reports"]]
    words = []
    for g, lad, ilen, snap, _ in jobs:
        words += ladder_words(g, lad, ilen, snap)
    out = run(fixture_exe, " ".join(str(x) for x in words))
    assert len(out) == len(jobs)
    for (g, lad, ilen, snap, ab), line in zip(jobs, out):
        (ev,), up, down, count, (complete,) = parse(line)
        rec = [U.num(v) for v in ab]
        assert complete == 1
        assert all(U.same_bits(up[i], rec[2 * i]) and U.same_bits(down[i], -rec[2 * i + 1]) for i in range(g["Nt"] - 1)), (g.get("name"), ilen, up, down, rec)
        m_ev, _, _, m_count = U.model_total(g, lad, ilen, snap=snap)
        assert U.same_bits(ev, m_ev) and [int(c) for c in count] == m_count
        if snap is not None:
            assert snap["lines"][0] == "Total log-evidence: " + M.g(ev)


@pytest.mark.parametrize("verbose", [1, 0])
def test_the_facades_records_print_the_reference_lines_and_keep_its_best_stderr(fixture_exe, verbose):
    lad = next(l for l in U.load()["long"] if l["verbose"] == verbose)
    totals = [U.model_total(lad, lad, lad["bin"], snap=rep)[0] for rep in lad["reports"]]
    out = run(fixture_exe, "records %d %d " % (len(totals), verbose) + " ".join(repr(v) for v in totals))
    at = 0
    for k, rep in enumerate(lad["reports"]):
        n = len(rep["lines"])
        assert out[at:at + n] == rep["lines"], (k, out[at:at + n], rep["lines"])
        assert out[at + n].startswith("best ") and U.same_bits(out[at + n][5:], U.num(rep["best"])), (k, out[at + n], rep["best"])
        at += n + 1
    assert at == len(out)


def recorded_and_computed(where, flags):
    """per recorded call of a group (or of the long ladders): (recorded answers, the model's under `flags`)"""
    if where == "long":
        for lad in U.load()["long"]:
            for rep in lad["reports"]:
                yield rep["query"]["ab"], (lambda lad=lad, rep=rep: U.pair_answers(lad, lad, lad["bin"], snap=rep, flags=flags))
    else:
        g = U.group(where)
        for lad in g["ladders"]:
            for q in lad["queries"]:
                yield q["ab"], (lambda lad=lad, q=q: U.pair_answers(g, lad, q["ilen"], flags=flags))


@pytest.mark.parametrize("name", sorted(U.WRONG))
def test_the_fixture_tells_each_wrong_reading_from_the_right_one(name):
    for where in U.WRONG[name]:
        with U.wrong_model(name) as flags:
            if name == "last_divisor_inverted":   # the ratios do not see it; the printed totals do
                changed = sum(rep["lines"][0] != "Total log-evidence: " + M.g(U.model_total(lad, lad, lad["bin"], snap=rep, flags=flags)[0])
                              for lad in U.load()["long"] for rep in lad["reports"])
                assert changed == 16
            else:
                changed = sum(U.differs(rec, comp) for rec, comp in recorded_and_computed(where, flags))
        assert changed > 0, (name, where)
    with U.wrong_model(name):
        pass
    assert all(not U.differs(rec, comp) for where in U.WRONG[name] for rec, comp in recorded_and_computed(where, U.RIGHT))   # the model is itself again


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_the_recorded_histories_in_the_engines_ring_numbering_give_the_recorded_ratios(name):
    """the reference's raw rows (Ninit initial rows in front) packed as the engine's ring holds them -- the start state row 0, slot =
    row mod capacity -- and read back by the model's ring reader with its Ninit = 1: the two numberings meet, wrapped or not"""
    g = U.group(name)
    nt, w_count, a = g["Nt"], len(g["ladders"]), g["add_every_N"]
    newest = max(U.ring_row(g, n - 1) for lad in g["ladders"] for n in lad["Nsize"])
    for cap in (newest + 3, newest):
        llike, row, nhist, beta = U.pack_ring(g, g["ladders"], cap)
        assert (row[:, nhist == nhist.max()].max() >= cap) == (cap == newest)
        for w, lad in enumerate(g["ladders"]):
            for q in lad["queries"]:
                ev, up, down, count = M.ring_total(llike, row, nhist, beta[w], nt, w_count, w, q["ilen"], a)
                rec = [U.num(v) for v in q["ab"]]
                assert all(U.same_bits(up[i], rec[2 * i]) and U.same_bits(down[i], -rec[2 * i + 1]) for i in range(nt - 1)), (cap, w, q["ilen"])
                assert U.same_bits(ev, U.model_total(g, lad, q["ilen"])[0])
    llike, row, nhist, beta = U.pack_ring(g, g["ladders"], 50 // a + 3)                   # a ring that lost the long windows
    with pytest.raises(LookupError):
        M.ring_total(llike, row, nhist, beta[0], nt, w_count, 0, min(g["ladders"][0]["Nhist"]), a)
