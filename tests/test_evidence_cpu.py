"""The log-evidence by thermodynamic integration without a GPU: the C ABI's new name, its refusal of null arguments before any device
is used, and the facade's evidence_estimator / evidence_records (tests/cxx/evidence_fixture_main.cc) against their plain-Python
restatement (tests/evidence_model.py), bit for bit."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import evidence_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_exports_and_binding_name_the_entry_point():
    from test_abi_cpu import declared_functions
    from ptmcmc_amd import engine as E
    assert "ptm_log_evidence" in declared_functions()
    assert "ptm_log_evidence" in E.EXPORTS
    assert hasattr(C.CDLL(E.LIB_PATH), "ptm_log_evidence")
    assert callable(E.Engine.log_evidence)


def test_entry_point_refuses_null_before_any_device_is_used():
    from ptmcmc_amd import engine as E
    L = E.load()
    ev = np.zeros(1)
    assert L.ptm_log_evidence(None, 10, ev.ctypes.data_as(C.POINTER(C.c_double)), None, None, None) == -1      # PTM_ERR_INVALID
    assert b"null argument" in L.ptm_last_error()


@pytest.fixture(scope="module")
def fixture_exe():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "evfx")
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ptmcmc_amd", "host"),
                               os.path.join(ROOT, "tests", "cxx", "evidence_fixture_main.cc"), "-L", os.path.join(ROOT, "ptmcmc_amd"), "-lptm_engine",
                               "-Wl,-rpath," + os.path.join(ROOT, "ptmcmc_amd"), "-pthread", "-o", exe])
        yield exe


def run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def same_bits(a, b):
    """equal doubles, bit for bit; the empty window's 0 / 0 is a NaN on both sides (its sign is the divider's own)"""
    a, b = float(a), float(b)
    return (math.isnan(a) and math.isnan(b)) or np.float64(a).tobytes() == np.float64(b).tobytes()


# (Nt, W, add_every_N, ilen, steps, evolving): the ladders of 2, 3 and 9 rungs; add_every_N 1 and 3 with ilen no multiple of it;
# the second-to-last is shorter than its window (Nhist < ilen); unequal Nhist inside a rung everywhere (the rung's walkers differ)
LADDERS = [(2, 1, 1, 50, 120, False), (3, 4, 1, 77, 200, False), (9, 5, 3, 100, 400, False), (3, 3, 3, 50, 173, True), (9, 2, 1, 64, 300, True),
           (3, 3, 1, 500, 200, False), (2, 2, 3, 7, 5, False)]


@pytest.mark.parametrize("case", LADDERS, ids=lambda c: "Nt%d_W%d_a%d_ilen%d_n%d%s" % (c[:5] + ("_evolving" if c[5] else "",)))
def test_estimator_equals_the_model_bit_for_bit(fixture_exe, case):
    nt, w_count, a, ilen, steps, evolving = case
    rng = np.random.default_rng(1000 * nt + 10 * w_count + a)
    nhist = [[steps + int(rng.integers(0, 9)) * (r > 0) + w * (r % 2) for w in range(w_count)] for r in range(nt)]   # [r][w]: a rung exchanged twice adds one more
    rows = [[(-20.0 * rng.random(1 + (nhist[r][w] - 1) // a + 1) * (1 + r)).tolist() for w in range(w_count)] for r in range(nt)]
    base = np.geomspace(1.0, 1.0 / 50, nt)
    beta = [[float(base[r] * (1 + (0.05 * rng.random() if evolving and 0 < r else 0))) for r in range(nt)] for _ in range(w_count)]
    words = ["ladder", nt, w_count, a, ilen]
    for r in range(nt):
        for w in range(w_count):
            words += [nhist[r][w], len(rows[r][w])] + [repr(v) for v in rows[r][w]]
    words += [repr(b) for bw in beta for b in bw]
    out = run(fixture_exe, " ".join(str(x) for x in words))
    assert len(out) == w_count
    short = 0
    for w, line in enumerate(out):
        ev_s, up_s, down_s, count_s, complete = [part.split() for part in line[2:].split("|")]
        ev, up, down, count = M.total([(lambda row, v=rows[r][w]: v[row]) for r in range(nt)], [nhist[r][w] for r in range(nt)], beta[w], ilen, a)
        assert complete == ["1"]
        assert [int(c) for c in count_s] == count, (w, count_s, count)
        assert same_bits(ev_s[0], ev), (w, ev_s, ev)
        assert all(same_bits(x, y) for x, y in zip(up_s, up)) and len(up_s) == nt - 1, (w, up_s, up)
        assert all(same_bits(x, y) for x, y in zip(down_s, down)) and len(down_s) == nt - 1, (w, down_s, down)
        short += count[0] == 0
        if steps >= ilen:
            assert math.isfinite(ev) and all(c == count[0] or abs(c - count[0]) <= 1 for c in count)
    assert (short == w_count) == (steps < ilen)          # Nhist < ilen (rung 0 has made `steps` adds): no row, 0 / 0


def test_window_leaves_the_newest_row_out_and_is_empty_for_a_short_chain():
    assert M.window(100, 10, 1) == (91, 100)            # rows of steps 90 .. 98: the row of step 99 (row 100) is left out
    assert M.window(100, 10, 3) == (31, 34)
    assert M.window(10, 10, 1) == (1, 10)
    assert M.window(9, 10, 1) == (9, 9)                 # Nhist < ilen: index -1 -> Nhist - 1, an empty window
    assert M.window(0, 10, 1) == (0, 0) and M.window(0, 10, 3) == (1, 1)


@pytest.mark.parametrize("verbose", [1, 0])
def test_records_print_the_model_lines_and_keep_its_best_stderr(fixture_exe, verbose):
    rng = np.random.default_rng(77)
    values = (-12.5 + 0.3 * rng.standard_normal(40)).tolist()
    out = run(fixture_exe, "records 40 %d " % verbose + " ".join(repr(v) for v in values))
    rec = M.Records()
    at = 0
    first_stderr = None
    for k, v in enumerate(values):
        lines = rec.push(v, bool(verbose))
        assert out[at:at + len(lines)] == lines, (k, out[at:at + len(lines)], lines)
        at += len(lines)
        assert out[at].startswith("best ") and same_bits(out[at][5:], rec.best), (k, out[at], rec.best)
        at += 1
        if first_stderr is None and rec.best < 1e100:
            first_stderr = k + 1
    assert at == len(out)
    assert first_stderr == 6 and 0 < rec.best < 0.3          # six epochs before the first standard error
    assert len(rec.records) == 5 and [len(r) for r in rec.records] == [39, 19, 9, 4, 1]
