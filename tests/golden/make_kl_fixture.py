"""Writes tests/golden/kl_divergence.json.gz: what the real reference answers for its proposal-test statistics
(test_proposal.hh: KL_divergence(P, Q, false), fake_KL_divergence, all_nnd2, one_nnd2) on a dozen pairs of sample sets.

Run by hand where the reference is mounted and the project is built (the objects under oracle/_ref/obj are linked):
    python tests/golden/make_kl_fixture.py /path/to/reference
No test runs this.  The sets are made here -- integers over a power of two, inside the wrapped domains, so that the reference's
enforcement changes nothing and the recorded sets are the ones it saw.  Before the file is written every named wrong reading of
tests/kl_model.py must miss some recorded answer, the model must reproduce every recorded distance and KL value bit for bit, and the
facade's kl_estimator likewise, and the largest relative difference of the model's and the facade's fake KL (another matrix inverse
than Eigen's) is measured and written into the header."""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import kl_model as K  # noqa: E402

SCALE = 2 ** 20


def grid(x):
    return np.round(np.asarray(x) * SCALE) / SCALE


def cases():
    rng = np.random.default_rng(20191)
    none = lambda dim: (np.zeros(dim, dtype=np.int32), np.zeros(dim), np.zeros(dim))
    out = []

    def add(name, P, Q, bounds=None):
        P, Q = grid(P), grid(Q)
        out.append(dict(name=name, P=P, Q=Q, bounds=bounds or none(P.shape[1])))

    add("dim1_smallest", rng.standard_normal((7, 1)), rng.standard_normal((7, 1)))
    add("dim1_unequal", rng.standard_normal((50, 1)), 1.5 * rng.standard_normal((31, 1)))
    q = rng.standard_normal((200, 2)) * [1.0, 2.0]
    add("dim2_shifted", q + [0.5, 0.0], q)
    w2 = (np.array([1, 0], dtype=np.int32), np.array([-1.0, 0.0]), np.array([3.0, 0.0]))
    add("dim2_wrapped", np.c_[rng.uniform(-1, 3, 100), rng.standard_normal(100)], np.c_[rng.uniform(-1, 3, 150), 1.2 * rng.standard_normal(150)], w2)
    add("dim5_unequal", rng.standard_normal((120, 5)), 1.3 * rng.standard_normal((80, 5)) + 0.2)
    w5 = (np.array([0, 1, 0, 1, 0], dtype=np.int32), np.array([0, -2.0, 0, 0.0, 0]), np.array([0, 2.0, 0, 8.0, 0]))
    P = rng.standard_normal((64, 5))
    Q = 1.1 * rng.standard_normal((200, 5))
    P[:, 1], Q[:, 1], P[:, 3], Q[:, 3] = rng.uniform(-2, 2, 64), rng.uniform(-2, 2, 200), rng.uniform(0, 8, 64), rng.uniform(0, 8, 200)
    add("dim5_wrapped", P, Q, w5)
    P = rng.standard_normal((60, 2))
    P[50:53], P[53:56] = P[0:3], P[0:3] + [0.0, 2.0 ** -18]          # three duplicated points, three nearly so
    Q = 1.2 * rng.standard_normal((45, 2))
    Q[0:2] = P[10:12]                                                 # two points of P are points of Q
    add("dim2_duplicates", P, Q)
    add("dim2_few_of_q", rng.standard_normal((7, 2)), rng.standard_normal((3, 2)) * 2)
    q = rng.standard_normal((200, 5))
    add("dim5_shifted", q + 0.25, q)
    w1 = (np.array([1], dtype=np.int32), np.array([0.0]), np.array([4.0]))
    add("dim1_wrapped", rng.uniform(0, 4, (40, 1)), np.r_[rng.uniform(0, 0.5, 20), rng.uniform(3.5, 3.999, 20)][:, None], w1)
    add("dim2_narrow", 0.7 * rng.standard_normal((150, 2)), rng.standard_normal((90, 2)))
    add("dim5_many_of_q", rng.standard_normal((30, 5)), rng.standard_normal((200, 5)) * 1.5)
    for c in out:
        w, lo, hi = c["bounds"]
        for d in range(c["P"].shape[1]):
            if w[d]:
                assert all(((s[:, d] >= lo[d]) & (s[:, d] < hi[d])).all() for s in (c["P"], c["Q"])), c["name"]
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REF")   # (oracle/Makefile's name for it)
    if not ref or not os.path.isdir(ref):
        sys.exit("usage: python tests/golden/make_kl_fixture.py /path/to/reference")
    objs = os.path.join(ROOT, "oracle", "_ref", "obj")
    cs = cases()
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "make_kl_fixture")
        subprocess.check_call(["g++", "-O2", "-g0", "-fopenmp", "-std=gnu++11", "-DHAVE_CXX11=1", "-w", "-I", ref, "-I", os.path.join(ref, "ProbabilityDist"),
                               "-I", os.path.join(ref, "eigen-eigen-323c052e1731"), os.path.join(HERE, "make_kl_fixture.cc")]
                              + sorted(os.path.join(objs, f) for f in os.listdir(objs) if f.endswith(".o")) + ["-o", exe])
        answers = K.parse_sets_output(K.run_driver(exe, K.sets_input(cs, head="")))
        facade = K.parse_sets_output(K.run_driver(K.build_fixture_driver(d), K.sets_input(cs)))       # the facade's kl_estimator
    assert len(answers) == len(cs)
    missed = {name: 0 for name in K.WRONG}
    rel, absolute, smallest = 0.0, 0.0, np.inf
    for c, a, fa in zip(cs, answers, facade):
        value, r, s = K.kl(c["P"], c["Q"], *c["bounds"], detail=True)
        assert K.same_bits(r, a["r"]) and K.same_bits(s, a["s"]) and K.same_bits(value, a["kl"]), (c["name"], value, a["kl"])
        assert K.same_bits(fa["r"], a["r"]) and K.same_bits(fa["s"], a["s"]) and K.same_bits(fa["kl"], a["kl"]), (c["name"], fa["kl"], a["kl"])
        for name, switches in K.WRONG.items():
            missed[name] += not K.same_bits(K.kl(c["P"], c["Q"], *c["bounds"], **switches), a["kl"])
        f = K.fake_kl(c["P"], c["Q"])
        for g in (f, fa["fkl"]):
            rel, absolute, smallest = max(rel, abs(g - a["fkl"]) / abs(a["fkl"])), max(absolute, abs(g - a["fkl"])), min(smallest, abs(a["fkl"]))
        print("%-18s kl %-22.17g fkl %-22.17g model %-22.17g facade %.17g" % (c["name"], a["kl"], a["fkl"], f, fa["fkl"]))
    print("wrong readings told apart in", missed, "of", len(cs), "cases")
    assert all(n > 0 for n in missed.values()), missed
    print("fake KL: largest relative difference %.3g, largest difference %.3g, smallest |value| %.3g" % (rel, absolute, smallest))
    assert absolute < 1e-6 * smallest
    fx = {
        "about": "test_proposal.hh of the real reference on sample sets: KL_divergence(P, Q, false), fake_KL_divergence(P, Q), all_nnd2(P), "
                 "one_nnd2(P[i], Q); coordinates are P_int / coordinate_scale, row-major [n][dim]",
        "coordinate_scale": SCALE,
        "fake_kl_model_max_rel_diff": rel,
        "fake_kl_model_max_abs_diff": absolute,
        "fake_kl_smallest_abs": smallest,
        "cases": [dict(name=c["name"], dim=int(c["P"].shape[1]), wrapped=[int(v) for v in c["bounds"][0]], xmin=[float(v) for v in c["bounds"][1]],
                       xmax=[float(v) for v in c["bounds"][2]], P_int=[int(v) for v in np.ravel(c["P"] * SCALE)], Q_int=[int(v) for v in np.ravel(c["Q"] * SCALE)],
                       kl=a["kl"], fake_kl=a["fkl"], r1sqs=[float(v) for v in a["r"]], s1sqs=[float(v) for v in a["s"]]) for c, a in zip(cs, answers)],
    }
    path = os.path.join(HERE, "kl_divergence.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(fx, separators=(",", ":")).encode())
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
