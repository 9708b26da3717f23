"""The log-evidence by thermodynamic integration over the ladder, restated in plain Python: sequential Python floats (IEEE doubles,
one rounding per operation) in the reference's order of operations.  What it restates:

  window    MH_chain::get_state_idx (chain.cc:1041-1049) of Nhist - ilen and Nhist, as parallel_tempering_chains::log_evidence_ratio
            calls it (chain.cc:1988-1989): an index outside [0, Nhist) becomes Nhist - 1; with Nzero = 0 the saved row of nominal
            step i is Ninit + i / add_every_N (C division).  The newest saved row is left out; Nhist < ilen gives an empty window.
            Ninit is the number of rows MH_chain::initialize(n) put in front (n of them, chain.cc:846-876).  The engine's ring calls
            the start state row 0 and the row of step i row 1 + i / add_every_N whatever n was -- further initial draws are kept in
            front of row 0 --, which is ninit = 1 here, the default.  The recorded ladders of tests/golden/evidence.json.gz
            (initialize(5), (3) among them) confirm that the two numberings meet: raw row = ring row + Ninit - 1, and no window
            reaches a row in front of Ninit.
  ratio     chain.cc:1990-2007: amb = beta_a - beta_b; x = llike_b[row] * amb; sum += x; count++; sum / count (0 / 0 = NaN).
  total     chain.cc:1585-1597: up[i] = ratio(i, i+1); down[i] = -ratio(i+1, i); evidence += (up[i] + down[i]) / 2.0; then
            evidence += (up[Nt-2] + down[Nt-2]) / 2.0 / (beta[Nt-2] / beta[Nt-1] - 1).
  records   chain.cc:1600-1675: the pyramid total_evidence_records, the "recent ev analysis", best_evidence_stderr (starts at 1e100,
            chain.hh) and the printed lines (std::cout's default format is C's %g).
The facade's evidence_estimator / evidence_records (ptmcmc_amd/host/ptmcmc_gpu.hh) and the device's kernels (ptm_log_evidence) must
give these very bits."""
import math

NAN = float("nan")


def cdiv(a, b):
    """C's integer division: towards zero"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def state_idx(i, nhist, add_every, ninit=1):
    if i < 0 or i >= nhist:
        i = nhist - 1
    return ninit + cdiv(i, add_every)


def window(nhist, ilen, add_every, ninit=1):
    return state_idx(nhist - ilen, nhist, add_every, ninit), state_idx(nhist, nhist, add_every, ninit)


def ratio(llike_of_row, nhist_b, beta_a, beta_b, ilen, add_every, ninit=1):
    """llike_of_row(row) -> float of chain b; returns (ratio, rows)"""
    first, last = window(nhist_b, ilen, add_every, ninit)
    amb = beta_a - beta_b
    total, count = 0.0, 0
    for row in range(first, last):
        x = llike_of_row(row) * amb
        total = total + x
        count += 1
    return (total / count if count else NAN), count


def total(readers, nhist, beta, ilen, add_every, ninit=1):
    """one ladder: readers[r](row) -> llike, nhist[r], beta[r].  Returns (evidence, up[Nt-1], down[Nt-1], count[Nt])"""
    nt = len(beta)
    up, down, count = [0.0] * (nt - 1), [0.0] * (nt - 1), [0] * nt
    evidence = 0.0
    for i in range(nt - 1):
        up[i], count[i + 1] = ratio(readers[i + 1], nhist[i + 1], beta[i], beta[i + 1], ilen, add_every, ninit)
        d, count[i] = ratio(readers[i], nhist[i], beta[i + 1], beta[i], ilen, add_every, ninit)
        down[i] = -d
        evidence = evidence + (up[i] + down[i]) / 2.0
    evidence = evidence + (up[nt - 2] + down[nt - 2]) / 2.0 / (beta[nt - 2] / beta[nt - 1] - 1)
    return evidence, up, down, count


def ring_reader(llike, row_of_slot, chain):
    """the engine's ring: llike[slot][chain], row_of_slot[slot][chain] the saved row number the slot holds"""
    cap = len(llike)

    def read(row):
        slot = row % cap
        if int(row_of_slot[slot][chain]) != row:
            raise LookupError("row %d of chain %d is not in the ring" % (row, chain))
        return float(llike[slot][chain])
    return read


def ring_total(llike, row_of_slot, nhist, beta_of, nt, w_count, w, ilen, add_every):
    """walker w's ladder on the engine's ring (chain = rung * W + walker); beta_of[r]: the chains' current inverse temperatures"""
    readers = [ring_reader(llike, row_of_slot, r * w_count + w) for r in range(nt)]
    return total(readers, [int(nhist[r * w_count + w]) for r in range(nt)], [float(b) for b in beta_of], ilen, add_every)


def g(x):
    """std::ostream << double with the default flags"""
    return "%g" % x


class Records:
    def __init__(self):
        self.records, self.count, self.dim, self.best = [], 0, 0, 1e100

    def push(self, evidence, verbose=True):
        out = ["Total log-evidence: " + g(evidence)]
        self.count += 1
        ndim = self.count.bit_length() - 1          # (int)log2(evidence_count)
        if ndim > self.dim:
            self.records.append([])
            self.dim += 1
        if self.dim > 0:
            self.records[0].append(evidence)
            out.append("total_evidence_records[0][%d]=%s" % (self.count - 2, g(evidence)))
        for i in range(1, self.dim):
            if self.count % (1 << i) == 0:
                out.append("i=%d ec=%d 1<<(i)=%d mod=%d" % (i, self.count, 1 << i, self.count % (1 << i)))
                lower = self.records[i - 1]
                self.records[i].append((lower[-2] + lower[-1]) / 2.0)
        if ndim > 0:
            out.append("total_log_evs:")
            ntot = len(self.records[0])
            ndisplay = min(ntot, 20 if verbose else -1)
            for i in range(ntot - ndisplay, ntot):
                line = ""
                for j in range(len(self.records)):
                    ind = (ntot + 1) // (1 << j) + (i - ntot) - 1
                    line += (g(self.records[j][ind]) if ind >= 0 else "      ---      ") + "\t"
                out.append(line)
        out.append("recent ev analysis:")
        nd = len(self.records)
        for j in range(nd - 1):
            nvar, n = 2 * (nd - j) + 1, len(self.records[j])
            if n < nvar:
                continue
            sum1 = sum2 = 0.0
            for ev in self.records[j][n - nvar:]:
                sum1 = sum1 + ev
                sum2 = sum2 + ev * ev
            mean = sum1 / nvar
            variance = (sum2 - sum1 * mean) / (nvar - 1)
            stderr = math.sqrt(variance / nvar) if variance >= 0 else NAN
            out.append("%d: N=%d <ev>=%s sigma=%s StdErr=%s" % (j, nvar, g(sum1 / nvar), g(math.sqrt(variance) if variance >= 0 else NAN), g(stderr)))
            if stderr < self.best:
                self.best = stderr
        return out
