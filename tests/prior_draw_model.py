"""Independent draws from the prior as a member of the proposal set (ptm_set_proposal_prior_draw), restated in plain Python from the
CPU oracle's exported primitives, the thermal reset_bins in plain floats, and a driver that steps the frozen oracle through a set
with such a member.

The move (the reference's draw_from_dist over the prior, proposal_distribution.hh:119-132):
  draw      dimension d from block d of the chain's stream (walker * Nt + rung) under tag 4 at the PT step; the block's words are used
            as the initial prior draw uses them: uniform  u01(v0) (hi - lo) + lo;  Gaussian  z0(v0, v1) sigma + x0;  polar / copolar
            the inverse cdf by 64 bisections on the oracle's cos / sin;  log  exp(u (log hi - log lo) + log lo)
  validity  the state is its own (not a sum on the current one): valid unless enforcing the boundaries fails
  ratio     log_hastings = lprior(current, as stored) - lprior(proposed, enforced)
  type      the member's index
The oracle knows no such member.  For a chain whose pick lands on it the driver installs a host proposal (Ladder.set_host_proposal)
that hands the oracle's MH step exactly this state, ratio, type and validity, and takes it away again; every other chain gets the
steering mixture of tests/adaptive_model.py.

Thermal shares (proposal_distribution.cc:37-59 with Tpow > 0): thresholds of a rung at inverse temperature beta,
  Tfac = 1 - beta ** Tpow;  shares /= sum;  bin_max[i] = last + shares[i];  bin_max[i] += (hot[i] - shares[i]) Tfac;  every bin_max /= bin_max[-1]
Every number is a Python float made by the same operations in the same order.
"""
import ctypes as C
import math

import numpy as np

import adaptive_model as AM
import oracle_lib as O

TAG_MH, TAG_SET, TAG_PRIOR = 0, 3, 4
# the split constants of the oracle's trigonometry (pi and pi/2 as a double plus the remainder)
PI_HI, PI_LO, HPI_HI = 3.141592653589793116e+00, 1.224646799147353207e-16, 1.570796326794896558e+00


def thermal_bins(shares, hot_shares, Tpow, beta):
    """reset_bins of a set at inverse temperature beta: (normalised shares, thresholds); hot_shares are normalised first, as the
    set's constructor does (proposal_distribution.cc:72-79)"""
    n = len(shares)
    shares = [float(s) for s in shares]
    hot = [float(h) for h in hot_shares]
    if Tpow > 0:
        hs = 0.0
        for h in hot:
            hs = hs + h
        hot = [h / hs for h in hot]
    Tfac = 0.0
    if Tpow > 0:
        Tfac = 1 - math.pow(beta, Tpow)
    total = 0.0
    for s in shares:
        total = total + s
    bins = [0.0] * n
    last = 0.0
    for i in range(n):
        shares[i] = shares[i] / total
        bins[i] = last + shares[i]
        if Tpow > 0:
            bins[i] = bins[i] + (hot[i] - shares[i]) * Tfac
        last = bins[i]
    top = bins[-1]
    return shares, [b / top for b in bins]


def _cos_0_pi(L, x):
    return L.ptmo_cos_hpi(x) if x <= HPI_HI else -L.ptmo_cos_hpi((PI_HI - x) + PI_LO)


def _sin_hpi(L, x):
    return L.ptmo_sin_0_pi(x) if x >= 0 else -L.ptmo_sin_0_pi(-x)


def draw_polar(u, lo, hi):
    L = O.lib()
    cl, ch = _cos_0_pi(L, lo), _cos_0_pi(L, hi)
    y = cl - u * (cl - ch)
    a, b = lo, hi
    for _ in range(64):
        m = 0.5 * (a + b)
        if _cos_0_pi(L, m) > y:
            a = m
        else:
            b = m
    return 0.5 * (a + b)


def draw_copolar(u, lo, hi):
    L = O.lib()
    sl, sh = _sin_hpi(L, lo), _sin_hpi(L, hi)
    y = sl + u * (sh - sl)
    a, b = lo, hi
    for _ in range(64):
        m = 0.5 * (a + b)
        if _sin_hpi(L, m) < y:
            a = m
        else:
            b = m
    return 0.5 * (a + b)


def draw_log(u, lo, hi):
    L = O.lib()
    l0 = L.ptmo_log(lo)
    return L.ptmo_exp(u * (L.ptmo_log(hi) - l0) + l0)


def prior_draw(pb, seed, stream, step):
    """the proposed state of chain `stream` at PT step `step`: [D] floats (before enforcing)"""
    L = O.lib()
    p = pb.p.contents
    x = np.zeros(pb.D)
    for d in range(pb.D):
        o = O.draw_block(seed, TAG_PRIOR, stream, step, d)
        t, lo, hi = p.ptype[d], p.plo[d], p.phi[d]
        if t == O.UNIFORM:
            x[d] = L.ptmo_u01(o[0]) * (hi - lo) + lo
        elif t == O.GAUSSIAN:
            x[d] = O.boxmuller(o[0], o[1])[0] * hi + lo
        elif t == O.POLAR:
            x[d] = draw_polar(L.ptmo_u01(o[0]), lo, hi)
        elif t == O.COPOLAR:
            x[d] = draw_copolar(L.ptmo_u01(o[0]), lo, hi)
        elif t == O.LOG:
            x[d] = draw_log(L.ptmo_u01(o[0]), lo, hi)
        else:
            x[d] = float("nan")
    return x


def prior_move(pb, seed, stream, step, lp_current):
    """(proposed state, log-Hastings ratio, validity): the ratio from the state as enforcing leaves it"""
    x = prior_draw(pb, seed, stream, step)
    ok, xe = pb.enforce(x)
    nlp = pb.lprior(xe, 1 if ok else 0)
    return x, lp_current - nlp, 1 if ok else 0


class FixedSet:
    """a set whose thresholds are given (one table per rung: ptm_set_proposal_mixture) and never move; the interface of
    adaptive_model.ChainSet"""

    def __init__(self, thresholds):
        self.bin_max = [float(t) for t in thresholds]
        self.K, self.K_inner, self.nested = len(self.bin_max), 0, -1

    def pick(self, x_top, x_inner, ready_top=None):
        x = x_top if self.K > 1 else 0.0
        for i in range(self.K):
            if (ready_top is None or ready_top(i)) and x < self.bin_max[i]:
                return i, -1, i
        raise RuntimeError("no member of the set is ready")

    def outcome(self, i, j, accepted):
        pass


def thermal_chain_set(top_shares, hot_shares, Tpow, beta, nested, inner_shares, rate_inner):
    """adaptive_model.ChainSet of a rung at inverse temperature beta whose top set (rate 0) has thermal thresholds: they enter the
    per-chain initial state and are never rebuilt"""
    cs = AM.ChainSet(top_shares, 0.0, nested, inner_shares, rate_inner)
    cs.top.shares, cs.top.bin_max = thermal_bins(top_shares, hot_shares, Tpow, beta)
    return cs


class PriorDrawOracle(AM.SteeredOracle):
    """SteeredOracle with member `prior_member` of the (top) set drawing from the prior.  chains[c]: the set of chain c in the ENGINE's
    order -- FixedSet or adaptive_model.ChainSet; scales / odfs [Nt][leaves] as for SteeredOracle (the prior member's are not read)."""

    def __init__(self, lad, seed, chains, scales, odfs, prior_member, de_init_extra=0):
        AM.SteeredOracle.__init__(self, lad, seed, chains, scales, odfs, de_init_extra)
        self.prior_member = prior_member
        self.moves = np.zeros(self.Nt * self.W, dtype=np.int64)         # Metropolis moves made with the prior member, engine order
        self._cur = None
        self._hook = O.make_propose_fn(self._propose)

    def _propose(self, X, rung, walker, step):
        r, w = int(rung[0]), int(walker[0])
        oc = w * self.Nt + r
        lp = float(self.lad.s.contents.lprior[oc])
        x, hast, valid = prior_move(self.lad.pb, self.seed, oc, step, lp)
        return x[None, :], [hast], [self.prior_member], [valid]

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
                base = lad._props[r]
                if i == self.prior_member:
                    L.ptmo_pt_set_host_proposal(lad.s, C.cast(self._hook, C.c_void_p), None)
                    L.ptmo_mh_step(lad.s, lad.pb.p, C.byref(base), lad.rng, w, r)
                    L.ptmo_pt_set_host_proposal(lad.s, None, None)
                    self.moves[r * W + w] += 1
                else:
                    mix = np.zeros(3 * nleaf)
                    for k in range(nleaf):
                        mix[3 * k] = -1.0 if k < leaf else 1.0
                        mix[3 * k + 1] = self.scales[r][k]
                        mix[3 * k + 2] = self.odfs[r][k]
                    prop = O._Proposal()
                    prop.kind, prop.M, prop.oneDfrac, prop.K = base.kind, base.M, base.oneDfrac, nleaf
                    prop.mix = mix.ctypes.data_as(O._dp)
                    L.ptmo_mh_step(lad.s, lad.pb.p, C.byref(prop), lad.rng, w, r)
                cs.outcome(i, j, lad.s.contents.last_accept_mh[oc] == 1)
            lad.s.contents.step += 1
