"""tests/golden/evidence.json.gz -- what the real reference answered for its thermodynamic-integration log-evidence (recorded by
oracle/ref_driver.cc golden-evidence) -- loaded once, the model of tests/evidence_model.py applied to its recorded rows, the named
wrong readings of chain.cc:1041-1049, 1585-1597 and 1984-2012 that the fixture must tell from the right one, and the recorded
histories packed into the engine's ring.

The fixture numbers a chain's saved llikes by the reference's RAW index: Ninit initial rows in front (MH_chain::initialize(n) adds n),
the row of step i at Ninit + i / add_every_N.  The engine's ring calls the last initial row (the start state) row 0: ring row = raw -
(Ninit - 1)."""
import contextlib
import functools
import gzip
import json
import math
import os

import numpy as np

import evidence_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
GROUPS = ("A", "B", "C", "D")


@functools.lru_cache(maxsize=None)
def load():
    with gzip.open(os.path.join(HERE, "golden", "evidence.json.gz"), "rt") as f:
        fx = json.load(f)
    scale = float(fx["llike_scale"])
    ladders = [lad for g in fx["groups"] for lad in g["ladders"]] + fx["long"]
    for lad in ladders:
        lad["llike"] = [[v / scale for v in rows] for rows in lad["llike64"]]      # exact: integers below 2^53 over a power of two
    return fx


def group(name):
    return next(g for g in load()["groups"] if g["name"] == name)


def num(v):
    """the driver's numbers: "nan" is a string"""
    return float(v)


def same_bits(a, b):
    a, b = float(a), float(b)
    return (math.isnan(a) and math.isnan(b)) or np.float64(a).tobytes() == np.float64(b).tobytes()


def raw_reader(rows):
    def read(raw):
        if raw < 0 or raw >= len(rows):
            raise LookupError("raw row %d of %d" % (raw, len(rows)))
        return rows[raw]
    return read


# ---- the named wrong readings ------------------------------------------------------------------------------------------------------
# name -> the groups in which it can act ("long": the two do_evid ladders).  Each is applied to the MODEL (its functions are replaced
# while the answers are computed); pair_answers / model_total below then give what a project with that mistake would compute.
WRONG = {
    "newest_row_included": GROUPS + ("long",),
    "start_one_row_early": GROUPS + ("long",),
    "start_one_row_late": GROUPS + ("long",),
    "ilen_counted_in_rows": ("B", "C", "D", "long"),           # add_every_N > 1
    "ninit_ignored": ("B", "C"),                               # initialize(5), initialize(3)
    "other_chains_llikes": GROUPS + ("long",),
    "sign_flipped": GROUPS + ("long",),
    "last_divisor_inverted": ("long",),                        # acts on the total only: the do_evid ladders print it
    "short_chain_clipped_not_emptied": GROUPS,                 # the queries with ilen > Nhist
    "nominal_temperatures": ("D",),                            # evolve_temps
}


@contextlib.contextmanager
def wrong_model(name):
    """the model with one named mistake; yields the flags pair_answers / model_total read"""
    flags = {"ninit_ignored": name == "ninit_ignored", "other_chain": name == "other_chains_llikes", "nominal": name == "nominal_temperatures"}
    saved = (M.window, M.ratio, M.total)
    window, ratio = M.window, M.ratio
    if name == "newest_row_included":
        M.window = lambda nh, ilen, a, ninit=1: (window(nh, ilen, a, ninit)[0], window(nh, ilen, a, ninit)[1] + 1)
    elif name == "start_one_row_early":
        M.window = lambda nh, ilen, a, ninit=1: (window(nh, ilen, a, ninit)[0] - 1, window(nh, ilen, a, ninit)[1])
    elif name == "start_one_row_late":
        M.window = lambda nh, ilen, a, ninit=1: (window(nh, ilen, a, ninit)[0] + 1, window(nh, ilen, a, ninit)[1])
    elif name == "ilen_counted_in_rows":
        M.window = lambda nh, ilen, a, ninit=1: window(nh, ilen * a, a, ninit)
    elif name == "short_chain_clipped_not_emptied":
        M.window = lambda nh, ilen, a, ninit=1: window(nh, min(ilen, nh), a, ninit)
    elif name == "sign_flipped":
        M.ratio = lambda ll, nh, ba, bb, ilen, a, ninit=1: ratio(ll, nh, bb, ba, ilen, a, ninit)
    elif name == "last_divisor_inverted":
        def total(readers, nhist, beta, ilen, a, ninit=1):
            ev, up, down, count = saved[2](readers, nhist, beta, ilen, a, ninit)
            nt = len(beta)
            last = (up[nt - 2] + down[nt - 2]) / 2.0
            partial = 0.0
            for i in range(nt - 1):
                partial = partial + (up[i] + down[i]) / 2.0
            return partial + last / (beta[nt - 1] / beta[nt - 2] - 1), up, down, count
        M.total = total
    elif name not in WRONG:
        raise KeyError(name)
    try:
        yield flags
    finally:
        M.window, M.ratio, M.total = saved


RIGHT = {"ninit_ignored": False, "other_chain": False, "nominal": False}


def _inputs(g, lad, snap, flags):
    """readers, Nhist, beta, add_every_N, Ninit of a ladder (snap: one report of a long ladder, else the ladder's end)"""
    snap = snap or lad
    readers = [raw_reader(rows) for rows in lad["llike"]]
    beta = [num(b) for b in (lad["invtemp0"] if flags["nominal"] else snap["invtemp"])]
    return readers, [int(n) for n in snap["Nhist"]], beta, int(g["add_every_N"]), (1 if flags["ninit_ignored"] else int(g["Ninit"]))


def pair_answers(g, lad, ilen, snap=None, flags=RIGHT):
    """[ratio(0, 1), ratio(1, 0), ratio(1, 2), ...] as the driver recorded them, from the model's ratio"""
    readers, nhist, beta, a, ninit = _inputs(g, lad, snap, flags)
    out = []
    for i in range(len(beta) - 1):
        up_from, down_from = (i, i + 1) if flags["other_chain"] else (i + 1, i)
        out.append(M.ratio(readers[up_from], nhist[up_from], beta[i], beta[i + 1], ilen, a, ninit)[0])
        out.append(M.ratio(readers[down_from], nhist[down_from], beta[i + 1], beta[i], ilen, a, ninit)[0])
    return out


def model_total(g, lad, ilen, snap=None, flags=RIGHT):
    """(evidence, up, down, count) of the model's total"""
    readers, nhist, beta, a, ninit = _inputs(g, lad, snap, flags)
    return M.total(readers, nhist, beta, ilen, a, ninit)


def differs(recorded, computed):
    """some recorded answer's bits are not reproduced (a row that does not exist counts: the reading asked for it)"""
    try:
        got = computed()
    except LookupError:
        return True
    return len(got) != len(recorded) or any(not same_bits(num(r), c) for r, c in zip(recorded, got))


# ---- the recorded histories in the engine's ring ------------------------------------------------------------------------------------
def ring_row(g, raw):
    return raw - (int(g["Ninit"]) - 1)


def pack_ring(g, ladders, cap, first_row=None):
    """the ladders as the walkers of one engine (chain = rung * W + walker): llike[cap][Nc], row[cap][Nc] with slot = ring row % cap,
    every chain's newest `cap` saved rows (from first_row on, if given); nhist[Nc], beta[W][Nt]"""
    nt, w_count = int(g["Nt"]), len(ladders)
    nc = nt * w_count
    llike, row = np.zeros((cap, nc)), np.full((cap, nc), -1, dtype=np.int32)
    nhist, beta = np.zeros(nc, dtype=np.int64), np.zeros((w_count, nt))
    for w, lad in enumerate(ladders):
        for r in range(nt):
            c = r * w_count + w
            rows = lad["llike"][r]
            newest = ring_row(g, len(rows) - 1)
            lo = max(0, newest - cap + 1, first_row if first_row is not None else 0)
            for rr in range(lo, newest + 1):
                llike[rr % cap, c] = rows[rr + int(g["Ninit"]) - 1]
                row[rr % cap, c] = rr
            nhist[c] = int(lad["Nhist"][r])
            beta[w, r] = num(lad["invtemp"][r])
    return llike, row, nhist, beta
