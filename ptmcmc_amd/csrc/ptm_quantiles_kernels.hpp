// ptm_quantiles_kernels.hpp -- exact posterior quantiles of a recorded rung, pooled over its walkers (ptm_quantiles,
// ptm_quantiles_series): the facade's quantile_estimator (ptmcmc_amd/host/ptmcmc_gpu.hh) restated for the device.  The reference
// runs one ladder and writes no quantiles: no reference counterpart.
//
// A chain is one walker's saved rows -- the history ring of a recorded rung, or a caller's plain array -- and its first nfeat
// parameters are the features.  Its window is its own newest nrows saved rows (ptm_rhat's rule).  The sample of a feature is the
// N = W * nrows values of the windows; they are ordered by the 64-bit key  u ^ (u >> 63 ? ~0 : 1 << 63)  of their bit pattern u
// (the order of the reals, -0 before +0, the infinities at the ends).  The definition (include/ptm_engine.h) asks for the order
// statistics s_lo and s_hi of every probability; an order statistic is a value of the sample, so any correct selection returns the
// same bits.  The distinct ranks asked for are the `slots` (at most 2 nq <= 64, ascending, the same for every feature).
//
// Selection by radix digits, the most significant first, QNT_BITS bits a pass, all features and all slots together:
//  - quantiles_bits_kernel: lane = w * ft + f of a tile of ft features, the feature fastest (moments_sum_kernel's walk; the permuted
//    32 / 64 / 128-dimension rows through ess_pos); grid.y splits the window's rows.  The bitwise AND and OR of a feature's keys:
//    per lane in registers, per workgroup in LDS (64-bit LDS atomics), then vector atomics on the global words.  Bits above the
//    highest one in which AND and OR differ (hb) are common to all keys -- a posterior is narrow: sign, exponent and leading
//    mantissa bits -- and the digits start below them.  AND == OR: the feature is constant and done.  CHECK: the ring has wrapped,
//    so a row is there only if its slot still names it; a missing row raises *flag and the caller throws everything away.
//  - quantiles_update_kernel: a workgroup per feature, a lane per slot.  pass < 0: hb, the first prefix (the common bits), the
//    ranks.  Otherwise a lane walks the 256 counts of its slot's histogram, finds the digit that holds its rank, appends it to its
//    prefix and takes the counts below it off its rank.  Slots whose prefixes are equal share one histogram, that of the first of
//    them (their leader).  It also leaves cand[f], the number of keys of the feature that are still candidates of a slot, and
//    clears the histograms for the next pass.
//  - quantiles_count_kernel: the walk of the first kernel; a key whose bits above the pass's digit equal a leader's prefix adds 1
//    to bin (feature, slot, digit) of the workgroup's histogram in LDS (32-bit LDS atomics; a workgroup sees fewer than 2^32 keys).
//    The histogram [features of a tile][slots][256] and the tile's prefixes fill at most QNT_LDS_BYTES of the CU's 160 KiB: the
//    features are tiled (grid.z).  Non-zero bins are merged into the 64-bit global counters with vector atomics.
//  - quantiles_pack_kernel: the same walk; the candidates of every feature are copied, as the doubles they are, into a plain
//    series [position][feature] in the workspace.  The passes after it read that series instead of the ring (`valid`: the
//    positions a feature has filled).  Where a key lands depends on the order of the atomics; the counts do not.
// A pass is one count launch and one update launch on the stream: no grid barrier, no flags.  Integer counts do not depend on the
// order of the adds, so every result is deterministic.  After the last pass a slot's prefix is the key of its order statistic; the
// interpolation is formed on the host.
// Plain vector loads, stores and atomics only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ptm_rhat_kernels.hpp"

namespace ptm {

constexpr int QNT_THREADS = 512;             // lanes per workgroup of the walking kernels
constexpr int QNT_AHEAD = 8;                 // rows whose loads are in flight before the first of their keys is used
constexpr int QNT_BITS = 8;                  // bits of a digit
constexpr int QNT_BINS = 1 << QNT_BITS;
constexpr int QNT_SLOTS_MAX = 64;            // distinct ranks: 2 nq at most
constexpr int QNT_STATE_MAX = 128;           // (feature, slot) pairs of a tile: 128 histograms of 1 KiB, 128 KiB of LDS
constexpr int QNT_LDS_BYTES = QNT_STATE_MAX * QNT_BINS * 4;
constexpr int QNT_PACK_WALKERS = 256;        // the packed series has this many "walkers": a position is row * 256 + walker

typedef unsigned long long qnt_u64;

__host__ __device__ inline qnt_u64 quantiles_key(qnt_u64 u) { return u ^ ((u >> 63) ? ~0ull : (1ull << 63)); }
__host__ __device__ inline qnt_u64 quantiles_unkey(qnt_u64 k) { return k ^ ((k >> 63) ? (1ull << 63) : ~0ull); }
// the bits of a key above bit `hi` (hi = 63: none)
__host__ __device__ inline qnt_u64 quantiles_above(qnt_u64 k, int hi) { return hi >= 63 ? 0ull : k >> (hi + 1); }

// what the walking kernels share: the lanes of tile blockIdx.z, the rows of chunk blockIdx.y
struct QntWalk {
  EssSrc src;
  const unsigned int* nhist;   // [walker] each chain's own count of add_state calls (null: src.steps for all)
  const long long* valid;      // [feature] the packed series: positions row * W + walker below it hold a key (null: every one does)
  long long room;              // ... and no position at or above this one does, whatever `valid` says
  int W, f0, nf, ft;           // walkers; the group's first feature in the source, its features, features of a tile
  int nrows, rows_per_chunk;
};

// walks the lane's rows and hands every key to use(key); false: a window the caller has not checked or a missing row
template <bool CHECK, class Use>
__device__ __forceinline__ bool quantiles_walk(const QntWalk& q, int w, int f, Use use) {
  // the window: ptm_rhat's rule (the caller has checked all of this: a lane never reads outside the ring)
  const long long steps = q.nhist ? (long long)q.nhist[w] : (long long)q.src.steps;
  const long long newest = q.src.first_row + (steps - 1) / q.src.add_every, first = newest - q.nrows + 1;
  if (steps < 1 || first < q.src.first_row || q.nrows > q.src.cap || (!CHECK && newest >= q.src.cap)) return false;
  const qnt_u64* xs = (const qnt_u64*)(q.src.x + (long long)w * q.src.series_stride + ess_pos(q.src, q.f0 + f));
  const int4* ms = CHECK ? q.src.meta + w : nullptr;
  const long long r0 = (long long)blockIdx.y * q.rows_per_chunk;
  const int n = (int)(q.nrows - r0 < q.rows_per_chunk ? q.nrows - r0 : q.rows_per_chunk);
  const long long have = q.valid ? (q.valid[f] < q.room ? q.valid[f] : q.room) : 0;
  bool missing = false;
  for (int i = 0; i < n; i += QNT_AHEAD) {
    qnt_u64 v[QNT_AHEAD];
    bool there[QNT_AHEAD];
#pragma unroll
    for (int j = 0; j < QNT_AHEAD; ++j) {
      there[j] = i + j < n && (!q.valid || (r0 + i + j) * q.W + w < have);
      const long long slot = there[j] ? rhat_slot<CHECK>(q.src, ms, first + r0 + i + j) : 0;
      if (slot < 0) { missing = true; there[j] = false; }
      v[j] = there[j] ? xs[slot * q.src.slot_stride] : 0ull;
    }
#pragma unroll
    for (int j = 0; j < QNT_AHEAD; ++j)
      if (there[j]) use(quantiles_key(v[j]));
  }
  return !missing;
}

// and_or[f], and_or[nf + f] &= / |= the keys of feature f (the caller has set them to ~0 and 0)
template <bool CHECK>
__global__ __launch_bounds__(QNT_THREADS) void quantiles_bits_kernel(QntWalk q, qnt_u64* __restrict__ and_or, int* __restrict__ flag) {
  __shared__ qnt_u64 and_s[QNT_STATE_MAX], or_s[QNT_STATE_MAX];
  const int tid = (int)threadIdx.x, fbase = (int)blockIdx.z * q.ft, ftc = q.nf - fbase < q.ft ? q.nf - fbase : q.ft;
  for (int i = tid; i < ftc; i += QNT_THREADS) { and_s[i] = ~0ull; or_s[i] = 0ull; }
  __syncthreads();
  const long long lane = (long long)blockIdx.x * QNT_THREADS + tid;
  if (lane < (long long)q.W * ftc) {
    const int w = (int)(lane / ftc), fl = (int)(lane - (long long)w * ftc);
    qnt_u64 a = ~0ull, o = 0ull;
    if (!quantiles_walk<CHECK>(q, w, fbase + fl, [&](qnt_u64 k) { a &= k; o |= k; })) *flag = 1;
    atomicAnd(&and_s[fl], a);
    atomicOr(&or_s[fl], o);
  }
  __syncthreads();
  for (int i = tid; i < ftc; i += QNT_THREADS) {
    atomicAnd(&and_or[fbase + i], and_s[i]);
    atomicOr(&and_or[q.nf + fbase + i], or_s[i]);
  }
}

// the selection's state of a group of nf features and ns slots
struct QntState {
  const long long* ranks;   // [ns] the distinct ranks, ascending
  qnt_u64* and_or;          // [2 nf]
  int* hb;                  // [nf] the highest bit in which the feature's keys differ; -1: a constant feature
  qnt_u64* prefix;          // [nf * ns] the bits of the slot's order statistic found so far (the common bits at first)
  long long* rank;          // [nf * ns] the slot's rank among the keys that share its prefix
  int* leader;              // [nf * ns] the first slot with the same prefix: the histogram the slot reads
  qnt_u64* hist;            // [nf * ns * QNT_BINS]
  long long* cand;          // [nf] keys that are still candidates of a slot
  int nf, ns;
};
// the digit of pass `pass` of a feature: bits lo .. hi of the key; hi < 0: the feature is done
__device__ __forceinline__ void quantiles_digit(int hb, int pass, int* hi, int* lo) {
  *hi = hb < 0 ? -1 : hb - QNT_BITS * pass;
  *lo = *hi - (QNT_BITS - 1) < 0 ? 0 : *hi - (QNT_BITS - 1);
}

// grid nf, QNT_SLOTS_MAX lanes.  flag: 2 if a rank lies outside its histogram (never, unless the kernels are wrong)
__global__ __launch_bounds__(QNT_SLOTS_MAX) void quantiles_update_kernel(QntState s, int pass, int* __restrict__ flag) {
  __shared__ qnt_u64 pref_s[QNT_SLOTS_MAX];
  __shared__ long long cand_s[QNT_SLOTS_MAX];
  const int f = (int)blockIdx.x, j = (int)threadIdx.x, at = f * s.ns + j;
  const bool mine = j < s.ns;
  bool live = false;   // the feature has digits left after this pass
  if (pass < 0) {
    const qnt_u64 a = s.and_or[f], diff = a ^ s.and_or[s.nf + f];
    const int hb = diff ? 63 - __clzll((long long)diff) : -1;
    if (j == 0) s.hb[f] = hb;
    if (mine) {
      pref_s[j] = hb < 0 ? a : (hb >= 63 ? 0ull : a & ~((1ull << (hb + 1)) - 1));
      cand_s[j] = 0;
      s.rank[at] = s.ranks[j];
    }
    live = hb >= 0;
  } else {
    int hi, lo;
    quantiles_digit(s.hb[f], pass, &hi, &lo);
    if (hi < 0) return;   // (the whole workgroup: done in an earlier pass, its histograms are clear)
    if (mine) {
      const qnt_u64* h = s.hist + ((size_t)f * s.ns + s.leader[at]) * QNT_BINS;
      const int bins = 1 << (hi - lo + 1);
      long long rank = s.rank[at], below = 0, c = 0;
      int d = -1;
      for (int b = 0; b < bins; ++b) {
        c = (long long)h[b];
        if (rank < below + c) { d = b; break; }
        below += c;
      }
      if (d < 0) { *flag = 2; d = 0; below = 0; c = 0; }
      pref_s[j] = s.prefix[at] | ((qnt_u64)d << lo);
      cand_s[j] = c;
      s.rank[at] = rank - below;
    }
    live = lo > 0;
  }
  __syncthreads();   // every histogram of the feature has been read
  if (mine) {
    int l = j;
    while (l > 0 && pref_s[l - 1] == pref_s[j]) --l;   // (the ranks ascend, so equal prefixes are neighbours)
    s.leader[at] = l;
    s.prefix[at] = pref_s[j];
    if (l != j) cand_s[j] = 0;
  }
  if (pass >= 0)
    for (int i = j; i < s.ns * QNT_BINS; i += QNT_SLOTS_MAX) s.hist[(size_t)f * s.ns * QNT_BINS + i] = 0ull;
  __syncthreads();
  if (j == 0) {
    long long total = 0;
    for (int k = 0; k < s.ns; ++k) total += cand_s[k];
    s.cand[f] = live ? total : 0;
  }
}

// the tile's prefixes, leaders and digit positions into LDS; returns the features of the tile
__device__ __forceinline__ int quantiles_tile_state(const QntWalk& q, const QntState& s, int pass, qnt_u64* pref_s, int* lead_s, int* hi_s) {
  const int tid = (int)threadIdx.x, fbase = (int)blockIdx.z * q.ft, ftc = q.nf - fbase < q.ft ? q.nf - fbase : q.ft;
  for (int i = tid; i < ftc * s.ns; i += QNT_THREADS) {
    pref_s[i] = s.prefix[(size_t)fbase * s.ns + i];
    lead_s[i] = s.leader[(size_t)fbase * s.ns + i];
  }
  for (int i = tid; i < ftc; i += QNT_THREADS) {
    int hi, lo;
    quantiles_digit(s.hb[fbase + i], pass, &hi, &lo);
    hi_s[i] = hi;
  }
  return ftc;
}
// the leader slot of feature-of-the-tile fl whose prefix the key carries above bit hi, or -1
__device__ __forceinline__ int quantiles_match(const qnt_u64* pref_s, const int* lead_s, int ns, int fl, int hi, qnt_u64 key) {
  const qnt_u64 above = quantiles_above(key, hi);
  for (int j = 0; j < ns; ++j)
    if (lead_s[fl * ns + j] == j && quantiles_above(pref_s[fl * ns + j], hi) == above) return j;
  return -1;
}

// dynamic LDS: ft * ns * QNT_BINS counters (q.ft * s.ns <= QNT_STATE_MAX)
template <bool CHECK>
__global__ __launch_bounds__(QNT_THREADS) void quantiles_count_kernel(QntWalk q, QntState s, int pass, int* __restrict__ flag) {
  extern __shared__ unsigned int qnt_hist_s[];
  __shared__ qnt_u64 pref_s[QNT_STATE_MAX];
  __shared__ int lead_s[QNT_STATE_MAX], hi_s[QNT_STATE_MAX];
  const int tid = (int)threadIdx.x, fbase = (int)blockIdx.z * q.ft;
  const int ftc = quantiles_tile_state(q, s, pass, pref_s, lead_s, hi_s), cells = ftc * s.ns * QNT_BINS;
  for (int i = tid; i < cells; i += QNT_THREADS) qnt_hist_s[i] = 0u;
  __syncthreads();
  const long long lane = (long long)blockIdx.x * QNT_THREADS + tid;
  if (lane < (long long)q.W * ftc) {
    const int w = (int)(lane / ftc), fl = (int)(lane - (long long)w * ftc), hi = hi_s[fl];
    if (hi >= 0) {
      const int lo = hi - (QNT_BITS - 1) < 0 ? 0 : hi - (QNT_BITS - 1);
      const unsigned mask = (1u << (hi - lo + 1)) - 1u;
      const bool ok = quantiles_walk<CHECK>(q, w, fbase + fl, [&](qnt_u64 k) {
        const int j = quantiles_match(pref_s, lead_s, s.ns, fl, hi, k);
        if (j >= 0) atomicAdd(&qnt_hist_s[(fl * s.ns + j) * QNT_BINS + (int)((unsigned)(k >> lo) & mask)], 1u);
      });
      if (!ok) *flag = 1;
    }
  }
  __syncthreads();
  for (int i = tid; i < cells; i += QNT_THREADS) {
    const unsigned c = qnt_hist_s[i];
    if (c) atomicAdd(&s.hist[(size_t)fbase * s.ns * QNT_BINS + i], (qnt_u64)c);
  }
}

// the candidates before pass `pass`: packed[position * nf + f], position drawn from fill[f]; positions >= room raise flag 2
template <bool CHECK>
__global__ __launch_bounds__(QNT_THREADS) void quantiles_pack_kernel(QntWalk q, QntState s, int pass, qnt_u64* __restrict__ fill, long long room,
                                                                     qnt_u64* __restrict__ packed, int* __restrict__ flag) {
  __shared__ qnt_u64 pref_s[QNT_STATE_MAX];
  __shared__ int lead_s[QNT_STATE_MAX], hi_s[QNT_STATE_MAX];
  const int tid = (int)threadIdx.x, fbase = (int)blockIdx.z * q.ft;
  const int ftc = quantiles_tile_state(q, s, pass, pref_s, lead_s, hi_s);
  __syncthreads();
  const long long lane = (long long)blockIdx.x * QNT_THREADS + tid;
  if (lane >= (long long)q.W * ftc) return;
  const int w = (int)(lane / ftc), fl = (int)(lane - (long long)w * ftc), hi = hi_s[fl];
  if (hi < 0) return;
  const bool ok = quantiles_walk<CHECK>(q, w, fbase + fl, [&](qnt_u64 k) {
    if (quantiles_match(pref_s, lead_s, s.ns, fl, hi, k) < 0) return;
    const qnt_u64 at = atomicAdd(&fill[fbase + fl], 1ull);
    if ((long long)at < room) packed[at * (qnt_u64)q.nf + (qnt_u64)(fbase + fl)] = quantiles_unkey(k);
    else *flag = 2;
  });
  if (!ok) *flag = 1;
}

}  // namespace ptm
