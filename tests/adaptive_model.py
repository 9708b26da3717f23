"""The adaptive proposal set (ptm_set_proposal_adaptive) restated in plain Python, and a driver that steers the frozen CPU oracle
through it step by step.

The rules are proposal_distribution_set's (the reference's proposal_distribution.cc:37-59, 99-166 with Tpow = 0; the facade's
proposal_distribution_set in ptmcmc_amd/host/ptmcmc_gpu.hh states them again):
  draw         a set of more than one member takes one uniform x; the pick is the first member that is ready with x < bin_max[i]
  accept/reject  for a set of rate != 0: a member whose outcome repeats its last one loses weight (share *= 1 - rate/4), its last
               outcome is stored, the outcome count goes up and -- from 10 x members outcomes on, the count is never reset -- the
               bins are rebuilt (reset_bins) after every outcome; the outcome is then handed to the picked member (a nested set)
  reset_bins   sum the shares in order, divide each by the sum, bin_max[i] = last + share[i], then every bin_max /= bin_max[-1]
Every number is a Python float (IEEE binary64) made by the same operations in the same order: no numpy reductions.

The oracle itself knows fixed mixtures only.  It is handed, for every chain and step, a STEERING mixture over the leaf table (the
top members, then the nested set's): cumulative shares -1 before the picked leaf and 1 from it on.  Its own Gaussian or
differential-evolution draw then takes exactly that leaf, with the leaf's scale and oneDfrac, from the same random streams as the
engine.  Its flat type code L + 10 t is mapped back to the nested code i + 10 (j + 10 t) by nested_type().
"""
import ctypes as C

import numpy as np

import oracle_lib as O

TAG_MH, TAG_SET = 0, 3


class AdaptiveSet:
    """one proposal_distribution_set's adaptive state for one chain"""

    def __init__(self, shares, rate):
        self.n = len(shares)
        self.shares = [float(s) for s in shares]
        self.bin_max = [0.0] * self.n
        self.last = [True] * self.n
        self.count = 0
        self.every = 10 * self.n
        self.rate = float(rate)
        self.reset_bins()

    def reset_bins(self):
        total = 0.0
        for s in self.shares:
            total = total + s
        last = 0.0
        for i in range(self.n):
            self.shares[i] = self.shares[i] / total
            self.bin_max[i] = last + self.shares[i]
            last = self.bin_max[i]
        top = self.bin_max[-1]
        for i in range(self.n):
            self.bin_max[i] = self.bin_max[i] / top

    def pick(self, x, ready=None):
        for i in range(self.n):
            if (ready is None or ready(i)) and x < self.bin_max[i]:
                return i
        raise RuntimeError("no member of the set is ready")

    def outcome(self, m, accepted):
        if self.rate == 0:
            return
        accepted = bool(accepted)
        if self.last[m] == accepted:
            self.shares[m] = self.shares[m] * (1 - self.rate * 0.25)
        self.last[m] = accepted
        self.count += 1
        if self.count >= self.every:
            self.reset_bins()

    def bits(self):
        b = 0
        for i in range(self.n):
            if self.last[i]:
                b |= 1 << i
        return b


class ChainSet:
    """the top set of K members, one of which (nested, or -1) is itself a set of K_inner Gaussians"""

    def __init__(self, top_shares, rate, nested=-1, inner_shares=None, rate_inner=0.0):
        self.top = AdaptiveSet(top_shares, rate)
        self.nested = nested
        self.inner = AdaptiveSet(inner_shares, rate_inner) if nested >= 0 else None
        self.K = self.top.n
        self.K_inner = self.inner.n if self.inner else 0

    def pick(self, x_top, x_inner, ready_top=None):
        i = self.top.pick(x_top if self.K > 1 else 0.0, ready_top)
        if i == self.nested:
            j = self.inner.pick(x_inner if self.K_inner > 1 else 0.0)
            return i, j, self.K + j
        return i, -1, i

    def outcome(self, i, j, accepted):
        self.top.outcome(i, accepted)
        if j >= 0:
            self.inner.outcome(j, accepted)

    def state(self):
        """weights, thresholds [K + K_inner]; repeat bits, outcome counts [2] (top, nested) -- ptm_get_proposal_adapt_state's row"""
        w, th = list(self.top.shares), list(self.top.bin_max)
        if self.inner:
            w += self.inner.shares
            th += self.inner.bin_max
        bits = [self.top.bits(), self.inner.bits() if self.inner else 0]
        cnt = [self.top.count, self.inner.count if self.inner else 0]
        return w, th, bits, cnt


def nested_type(flat, K, nested):
    """the oracle's flat leaf code L + 10 t -> the adaptive set's i + 10 t (top member) or i + 10 (j + 10 t) (nested member j)"""
    flat = int(flat)
    L, t = flat % 10, flat // 10
    if flat < 0 or L < K:   # (-1: nothing accepted yet)
        return flat
    return nested + 10 * ((L - K) + 10 * t)


def states_of(chains):
    """the per-chain state of a list of ChainSets as numpy arrays (the engine's layout)"""
    rows = [c.state() for c in chains]
    w = np.array([r[0] for r in rows], dtype=np.float64)
    th = np.array([r[1] for r in rows], dtype=np.float64)
    bits = np.array([r[2] for r in rows], dtype=np.int32)
    cnt = np.array([r[3] for r in rows], dtype=np.int32)
    return w, th, bits, cnt


class SteeredOracle:
    """The oracle ladder `lad` (set_proposals done, philox rng, optional DE and history) driven through per-chain adaptive sets.
    chains[c] is the set of chain c in the ENGINE's order (c = r * W + w); leaves [Nt][L][2] = {scale, oneDfrac}."""

    def __init__(self, lad, seed, chains, scales, odfs, de_init_extra=0):
        self.lad, self.seed = lad, seed
        self.Nt, self.W, self.D = lad.Nt, lad.W, lad.D
        self.chains = chains
        self.scales = np.asarray(scales, dtype=np.float64)
        self.odfs = np.asarray(odfs, dtype=np.float64)
        self.de_init_extra = de_init_extra
        self.de_on = bool(lad.s.contents.de_on)
        self.K = chains[0].K
        self.nested = chains[0].nested

    def _ready(self, oc, r, nsize):
        rows = self.de_init_extra + int(nsize[oc])
        def ready(i):
            if not self.de_on or i == self.nested or not (self.scales[r][i] < 0):
                return True
            return rows >= 10 * self.D
        return ready

    def sweep(self, n=1):
        """plain MH sweeps: every chain moves, no exchange phase"""
        self.step(n, exchange=False)

    def step(self, n=1, exchange=True):
        L = O.lib()
        lad = self.lad
        Nt, W = self.Nt, self.W
        N = Nt * W
        nleaf = self.scales.shape[1]
        for _ in range(n):
            if exchange:
                L.ptmo_exchange_phase(lad.s, lad.rng)
                touched = np.ctypeslib.as_array(lad.s.contents.touched, shape=(N,)).copy()
            else:
                touched = np.zeros(N, dtype=np.uint8)
            nsize = lad.nsize
            step = lad.step
            for oc in range(N):
                w, r = divmod(oc, Nt)
                if touched[oc]:
                    lad.s.contents.last_accept_mh[oc] = 2
                    continue
                cs = self.chains[r * W + w]
                x_top = L.ptmo_u01(O.draw_block(self.seed, TAG_MH, oc, step, 0)[3])
                x_in = L.ptmo_u01(O.draw_block(self.seed, TAG_SET, oc, step, 0)[0])
                i, j, leaf = cs.pick(x_top, x_in, self._ready(oc, r, nsize))
                mix = np.zeros(3 * nleaf)
                for k in range(nleaf):
                    mix[3 * k] = -1.0 if k < leaf else 1.0
                    mix[3 * k + 1] = self.scales[r][k]
                    mix[3 * k + 2] = self.odfs[r][k]
                base = lad._props[r]
                prop = O._Proposal()
                prop.kind, prop.M, prop.oneDfrac, prop.K = base.kind, base.M, base.oneDfrac, nleaf
                prop.mix = mix.ctypes.data_as(O._dp)
                L.ptmo_mh_step(lad.s, lad.pb.p, C.byref(prop), lad.rng, w, r)
                cs.outcome(i, j, lad.s.contents.last_accept_mh[oc] == 1)
            lad.s.contents.step += 1

    def state(self):
        return states_of(self.chains)

    def last_type(self):
        """the oracle's last_type in the engine's order, mapped to the nested codes"""
        lt = self.lad.last_type
        out = np.empty(self.Nt * self.W, dtype=np.int64)
        for oc in range(self.Nt * self.W):
            w, r = divmod(oc, self.Nt)
            out[r * self.W + w] = nested_type(lt[oc], self.K, self.nested)
        return out
