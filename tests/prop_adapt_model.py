"""The facade's gaussian_prop::eigen_factor (ptmcmc_amd/host/ptmcmc_gpu.hh: detail::jacobi_eigen, its swap sort, F = V sqrt(max(lambda,
0))) and the status rule of ptm_adapt_proposals restated in Python: the checker of ptm_eigen_factors and ptm_adapt_proposals (the
definition stands in include/ptm_engine.h).

Every floating-point operation is the C++ one, in its order.  The rotation is decided in scalar float64 arithmetic; each of its three
loops runs over independent elements k, so it is one elementwise numpy expression (multiply, multiply, subtract: no fused operation).
The off-diagonal sum is an explicit sequential loop.  `variant` names a deliberate misreading, for the test that shows the comparison
can tell them apart.
"""
import math

import numpy as np

SWEEPS_MAX = 100
SIZES = (1, 2, 3, 6, 17, 32, 33, 64, 65, 128)
KINDS = ("spd", "identity", "descending", "repeated", "rank", "tiny_off", "huge", "nan")
SPD_KINDS = ("spd", "descending", "repeated")     # symmetric positive definite with something to rotate or to sort


def _off(A, n):
    """0.0 + A[0][1]^2 + A[0][2]^2 + ... over p < q in that order, one term after the other"""
    off = 0.0
    for p in range(n - 1):
        row = A[p, p + 1:]
        for v in (row * row).tolist():
            off += v
    return off


def rotations(C, rows_first=False):
    """(A, Q, sweeps) when detail::jacobi_eigen's sweeps are over: the rotated matrix, the accumulated rotations, the sweeps that rotated"""
    A = np.array(C, dtype=np.float64)
    n = A.shape[0]
    Q = np.eye(n)
    sweeps, last = SWEEPS_MAX, None
    with np.errstate(all="ignore"):
        for sweep in range(SWEEPS_MAX):
            if _off(A, n) < 1e-300:
                sweeps = sweep
                break
            if np.isnan(A).all() and np.isnan(Q).all():
                break          # (every further rotation reads NaN and writes NaN: the remaining sweeps change nothing)
            before = A.tobytes() + Q.tobytes()
            if sweep and before == last:
                break          # (a sweep that changed no bit: a sweep is a function of A and Q alone, so no later one changes any)
            last = before
            for p in range(n):
                for q in range(p + 1, n):
                    apq = np.float64(A[p, q])
                    if abs(apq) < 1e-300:
                        continue
                    theta = (np.float64(A[q, q]) - np.float64(A[p, p])) / (np.float64(2) * apq)
                    t = np.float64(1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + np.float64(1)))
                    c = np.float64(1) / np.sqrt(t * t + np.float64(1))
                    sn = t * c

                    def columns(M):
                        a, b = M[:, p].copy(), M[:, q].copy()
                        M[:, p] = c * a - sn * b
                        M[:, q] = sn * a + c * b

                    def rows(M):
                        a, b = M[p, :].copy(), M[q, :].copy()
                        M[p, :] = c * a - sn * b
                        M[q, :] = sn * a + c * b

                    if rows_first:
                        rows(A)
                        columns(A)
                    else:
                        columns(A)
                        rows(A)
                    columns(Q)
    return A, Q, sweeps


def jacobi(C, variant=None, done=None):
    """(lambda[n] ascending by the swap sort, V[n, n], sweeps) of symmetric C as detail::jacobi_eigen gives them; done: rotations(C)"""
    A, Q, sweeps = done if done is not None else rotations(C, rows_first=variant == "rows_first")
    n = A.shape[0]
    order = list(range(n))
    if variant != "no_sort":
        for i in range(n):
            for j in range(i + 1, n):
                if A[order[j], order[j]] < A[order[i], order[i]]:
                    order[i], order[j] = order[j], order[i]
    lam = np.array([A[o, o] for o in order], dtype=np.float64)
    return lam, Q[:, order].copy(), sweeps


def eigen_factor(C, variant=None, done=None):
    """(F[n, n], lambda[n], sweeps): F[i][j] = V[i][j] * sqrt(lambda_j > 0 ? lambda_j : 0)"""
    lam, V, sweeps = jacobi(C, variant, done)
    with np.errstate(all="ignore"):
        sg = np.sqrt(lam if variant == "unclipped" else np.where(lam > 0, lam, 0.0))
        return V * sg[None, :], lam, sweeps


def dense_status(C, lam):
    """0: install; 1: an entry of the covariance is not finite; 2: the smallest eigenvalue is not above 0"""
    if not np.isfinite(C).all():
        return 1
    return 0 if lam[0] > 0 else 2


def diag_status(var):
    if not np.isfinite(var).all():
        return 1
    return 0 if (var > 0).all() else 2


def adapt(cov_or_var, scale, diag=False):
    """(factor, status) of one rung as ptm_adapt_proposals forms them: scale * F (one multiply per element) or scale * sqrt(var)"""
    with np.errstate(all="ignore"):
        if diag:
            v = np.asarray(cov_or_var, dtype=np.float64)
            return np.float64(scale) * np.sqrt(v), diag_status(v)
        F, lam, _ = eigen_factor(cov_or_var)
        return np.float64(scale) * F, dense_status(np.asarray(cov_or_var), lam)


def same_bits(a, b):
    """equal bit for bit, a NaN of any payload standing for a NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all()) and a[~na].tobytes() == b[~nb].tobytes()


# ---- the test matrices --------------------------------------------------------------------------------------------------------
# Built from the generator's normals by elementwise operations and sequential sums alone (no BLAS, no LAPACK), so that every machine
# makes the same bits and the recorded answers (tests/golden/prop_adapt_hashes.json) can stand for the twin where running it would take
# minutes (100 sweeps at 128 dimensions are 812800 rotations).
# the seed of each size's rank n - 1 matrix: the first for which the smallest eigenvalue comes out below 0, so that the clip acts
RANK_SEED = {1: 0, 2: 0, 3: 3, 6: 3, 17: 0, 32: 3, 33: 1, 64: 0, 65: 2, 128: 2}


def _gram(B, d=None):
    """sum over k, one term after the other, of d[k] * outer(B[:, k], B[:, k]): symmetric to the bit"""
    C = np.zeros((B.shape[0], B.shape[0]))
    for k in range(B.shape[1]):
        o = B[:, k][:, None] * B[:, k][None, :]
        C = C + (o if d is None else d[k] * o)
    return C


def matrix(kind, n, seed=0):
    rng = np.random.default_rng(1000 * n + seed)
    if kind == "spd":
        return _gram(rng.standard_normal((n, n + 3))) / float(n + 3)
    if kind == "identity":
        return np.eye(n)
    if kind == "descending":       # already diagonal: nothing rotates, the sort must act
        return np.diag(np.arange(n, 0, -1, dtype=np.float64) * 0.75)
    if kind == "repeated":         # eigenvalues 3 (n // 2 times) and 1 in the frame of a Householder reflection
        v = rng.standard_normal(n)
        H = np.eye(n) - (2.0 / math.fsum((v * v).tolist())) * (v[:, None] * v[None, :])
        return _gram(H, np.where(np.arange(n) < n // 2, 3.0, 1.0))
    if kind == "rank":             # rank n - 1: one eigenvalue is 0 up to rounding (n = 1: exactly 0)
        rng = np.random.default_rng(1000 * n + 500 + RANK_SEED.get(n, 0) + seed)
        return _gram(rng.standard_normal((n, n - 1))) if n > 1 else np.zeros((1, 1))
    if kind == "tiny_off":         # off-diagonals of 1e-305: each rotation is skipped, the first off sum ends the iteration
        C = np.full((n, n), 1e-305)
        C[np.arange(n), np.arange(n)] = rng.uniform(0.5, 2.0, size=n)
        return C
    if kind == "huge":             # diagonal near 1e150 beside small off-diagonals: theta * theta overflows
        C = matrix("spd", n, seed) * 1e-6
        C[np.arange(n), np.arange(n)] = rng.uniform(1.0, 2.0, size=n) * 1e150 * (1 + np.arange(n))
        return C
    if kind == "nan":
        C = matrix("spd", n, seed)
        C[0, min(1, n - 1)] = C[min(1, n - 1), 0] = np.nan
        return C
    raise ValueError(kind)


_cache = {}


def reference(kind, n):
    """(C, F, lambda, sweeps, status) of a test matrix by the twin, computed once"""
    key = (kind, n)
    if key not in _cache:
        C = matrix(kind, n)
        done = rotations(C)
        F, lam, sw = eigen_factor(C, done=done)
        _cache[key] = (C, F, lam, sw, dense_status(C, lam), done)
    return _cache[key][:5]


def reference_rotations(kind, n):
    reference(kind, n)
    return _cache[(kind, n)][5]


def digest(a):
    """sha256 of the array's bits, every NaN standing for the same NaN"""
    import hashlib
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = np.nan
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


GOLDEN = "prop_adapt_hashes.json"


def golden():
    """the twin's recorded answers: {"kind:n": {"input", "F", "lambda": digests; "sweeps", "status"}} (python tests/prop_adapt_model.py
    records them; tests/test_prop_adapt_model_cpu.py holds the twin to them)"""
    import json
    import os
    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)))


def record(kind, n):
    C, F, lam, sw, st = reference(kind, n)
    return {"input": digest(C), "F": digest(F), "lambda": digest(lam), "sweeps": int(sw), "status": int(st)}


# ---- the facade's own answers (tests/cxx/prop_adapt_main.cc) --------------------------------------------------------------------
def build_fixture_driver(d, sanitize=False):
    """tests/cxx/prop_adapt_main.cc: gaussian_prop's factor and jacobi_eigen's eigenvalues for matrices piped to it (no device).
    sanitize: built with the address and undefined-behaviour sanitizers (a stand-alone host program)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(d, "prop_adapt_fx_san" if sanitize else "prop_adapt_fx")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++11"] + flags + ["-ffp-contract=off", "-Wall", "-I", os.path.join(root, "include"), "-I", os.path.join(root, "ptmcmc_amd", "host"),
                           os.path.join(root, "tests", "cxx", "prop_adapt_main.cc"), "-pthread", "-o", exe])
    return exe


def fixture_driver_answers(exe, mats):
    """[(F, lambda)] of the fixture program for a list of square matrices; hex doubles both ways"""
    import subprocess
    lines = ["%d" % len(mats)]
    for C in mats:
        C = np.asarray(C, dtype=np.float64)
        lines.append("%d" % C.shape[0])
        lines.append(" ".join(float(v).hex() for v in C.ravel()))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = out.stdout.strip().splitlines()
    assert len(rows) == 2 * len(mats)
    res = []
    for k, C in enumerate(mats):
        n = np.asarray(C).shape[0]
        F = np.array([float.fromhex(v) for v in rows[2 * k].split()[1:]]).reshape(n, n)
        lam = np.array([float.fromhex(v) for v in rows[2 * k + 1].split()[1:]])
        res.append((F, lam))
    return res


if __name__ == "__main__":
    import json
    import os
    out = {"%s:%d" % (k, n): record(k, n) for n in SIZES for k in KINDS}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)
    json.dump(out, open(path, "w"), indent=0, sort_keys=True)
    print("recorded", len(out), "answers in", path)
