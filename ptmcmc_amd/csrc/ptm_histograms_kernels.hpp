// ptm_histograms_kernels.hpp -- the corner plot's counts of a recorded rung, pooled over its walkers (ptm_histograms,
// ptm_histograms_series): the 1-D histogram of every feature and the 2-D histogram of every pair of features, the facade's
// histogram_estimator (ptmcmc_amd/host/ptmcmc_gpu.hh) restated for the device.  The reference bins on the host with numpy
// (python/corner_with_covar.py): no device counterpart.
//
// A chain is one walker's saved rows -- the history ring of a recorded rung, or a caller's plain array -- and its first nfeat
// parameters are the features.  Its window is its own newest nrows saved rows (ptm_rhat's rule, ptm_quantiles' sample).  The
// definition (include/ptm_engine.h) is the edges: edge_k = lo + (double)k * step, step = (hi - lo) / (double)nbins, edge_nbins = hi;
// x lies in bin k iff edge_k <= x < edge_{k+1}, the last bin closed.  histograms_bin lands every double in that bin: a guess from
// one multiply, then a look at the two edges around it, formed by the definition's own expression (the engine is compiled with
// -ffp-contract=off: multiply, then add); a guess that is off -- by one near an edge, by anything in a range a few hundred ulps
// wide -- is put right by a bisection over the same edges, seven steps at most.
//  - histograms_1d_kernel: quantiles_walk's lanes, lane = w * ft + f of a tile of ft features (grid.z), the feature fastest; grid.y
//    splits the window's rows.  A value adds 1 to counter (feature, bin) of the workgroup's table in LDS, [ft][nbins + 2] 32-bit
//    counters (integer LDS atomics; a workgroup sees fewer than 2^32 values); the two counters behind a feature's bins are its
//    `below` and `above`.  Non-zero counters are merged into the 64-bit global ones with vector atomics.
//  - histograms_2d_kernel: grid.x: blocks of HIST_WALKERS walkers, grid.y: chunks of rows, grid.z: tiles of tp consecutive pairs.
//    The tile's tables [tp][nbins * nbins] of 32-bit counters fill at most HIST_TABLE_BYTES of the CU's 160 KiB (HistLds).  A
//    sample is one saved row of one walker.  The workgroup stages the bin indices of HistLds::samples samples at a time, a byte a
//    feature (255: outside its range, a NaN, or no sample), the feature fastest, then the walker: consecutive lanes read consecutive
//    doubles of the ring, and HIST_AHEAD loads of a lane are asked before the first is binned.  Then the (sample, pair) adds are
//    dealt to the lanes, by one of two mappings:
//      HIST_MAP_PAIRS  item = sample * tp + pair: the lanes of a wave hold different pairs of one sample (of two, three ... where tp
//                      is below 64), so no two of them add to the same counter unless two samples do;
//      HIST_MAP_ROWS   item = pair * samples + sample: the lanes of a wave hold different samples of one pair, and add to the same
//                      counter wherever the posterior is peaked.
//    A pair one of whose two values lies outside its range is left out (np.histogram2d's rule).  Non-zero counters are merged into
//    the 64-bit global tables with vector atomics: one global atomic per non-zero bin per workgroup.
// CHECK: the ring has wrapped, so a row is there only if its slot still names it; a missing row raises *flag and the caller throws
// everything away.  Integer counts do not depend on the order of the adds, so every result is deterministic, and the same whatever
// the tile, the mapping and the grid.
// Plain vector loads, stores and atomics only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ptm_lds_layout.hpp"
#include "ptm_quantiles_kernels.hpp"

namespace ptm {

constexpr int HIST_BINS_MAX = 128;
constexpr int HIST_THREADS = 1024;            // lanes per workgroup of the 2-D kernel (the 1-D kernel: QNT_THREADS)
constexpr int HIST_AHEAD = QNT_AHEAD;         // loads of a lane in flight before the first of their values is binned
constexpr int HIST_WALKERS = 64;              // walkers of a workgroup of the 2-D kernel
constexpr int HIST_FEATS = 64;                // features of a tile of the 1-D kernel: 64 * 130 counters, 33 KiB at most
constexpr int HIST_BLOCKS = 1024;             // workgroups of a launch, about: four for each of the chip's 256 CUs
constexpr int HIST_TABLE_BYTES = QNT_LDS_BYTES;   // the counters of a tile: 128 KiB of the CU's 160 KiB, the quantiles kernels' budget
constexpr int HIST_STAGE_BYTES = 8192;        // staged bin indices: at least one sample of the 8192 features 2^25 counters allow
constexpr int HIST_PAIRS_MAX = 2048;          // pairs of a tile (their list: 8 KiB)
constexpr int HIST_OUTSIDE = 255;             // the staged index of a value outside its range
constexpr int HIST_MAP_PAIRS = 0, HIST_MAP_ROWS = 1;
constexpr long long HIST_CELLS_MAX = 1ll << 25;   // npairs * nbins * nbins: 256 MiB of 64-bit counters

// a feature's range as the kernels read it: [4 f + 0 .. 3] = lo, hi, step = (hi - lo) / nbins, nbins / (hi - lo)
constexpr int HIST_PAR = 4;

// edge k of nbins + 1: the definition's expression -- multiply, then add -- and the last edge is hi itself
__host__ __device__ inline double histograms_edge(double lo, double hi, double step, int nbins, int k) {
  if (k >= nbins) return hi;
  const double up = (double)k * step;
  return lo + up;
}
// the bin of x: 0 .. nbins - 1; nbins: below lo; nbins + 1: above hi; -1: a NaN
__host__ __device__ inline int histograms_bin(double x, double lo, double hi, double step, double inv, int nbins) {
  if (x != x) return -1;
  if (x < lo) return nbins;
  if (x > hi) return nbins + 1;
  if (x == hi) return nbins - 1;   // the last bin is closed
  const double t = (x - lo) * inv;
  int k = t >= 0.0 ? (t < (double)nbins ? (int)t : nbins - 1) : 0;   // (a NaN or a negative guess: bin 0)
  if (histograms_edge(lo, hi, step, nbins, k) <= x && x < histograms_edge(lo, hi, step, nbins, k + 1)) return k;
  // the largest k with edge_k <= x (edge_0 = lo <= x < hi = edge_nbins, the edges strictly increasing)
  int a = 0, b = nbins - 1;
  while (a < b) {
    const int mid = (a + b + 1) >> 1;
    if (histograms_edge(lo, hi, step, nbins, mid) <= x) a = mid;
    else b = mid - 1;
  }
  return a;
}
// pair p of the upper triangle in row-major order: i < j
__host__ __device__ inline void histograms_pair(int nfeat, long long p, int* i, int* j) {
  int a = 0;
  long long left = p;
  while (left >= nfeat - 1 - a) { left -= nfeat - 1 - a; ++a; }
  *i = a;
  *j = a + 1 + (int)left;
}

// ---- the 1-D kernel ----------------------------------------------------------------------------------------------------------------
// dynamic LDS: q.ft * (nbins + 2) counters.  h1: [q.nf][nbins + 2] global counters of the group's features.
template <bool CHECK>
__global__ __launch_bounds__(QNT_THREADS) void histograms_1d_kernel(QntWalk q, const double* __restrict__ par, int nbins, qnt_u64* __restrict__ h1,
                                                                   int* __restrict__ flag) {
  extern __shared__ unsigned int hist1_s[];
  const int tid = (int)threadIdx.x, fbase = (int)blockIdx.z * q.ft, ftc = q.nf - fbase < q.ft ? q.nf - fbase : q.ft;
  const int cells = ftc * (nbins + 2);
  for (int i = tid; i < cells; i += QNT_THREADS) hist1_s[i] = 0u;
  __syncthreads();
  const long long lane = (long long)blockIdx.x * QNT_THREADS + tid;
  if (lane < (long long)q.W * ftc) {
    const int w = (int)(lane / ftc), fl = (int)(lane - (long long)w * ftc);
    const double* pf = par + (size_t)HIST_PAR * (size_t)(q.f0 + fbase + fl);
    const double lo = pf[0], hi = pf[1], step = pf[2], inv = pf[3];
    unsigned int* mine = hist1_s + fl * (nbins + 2);
    const bool ok = quantiles_walk<CHECK>(q, w, fbase + fl, [&](qnt_u64 key) {
      const int k = histograms_bin(__longlong_as_double((long long)quantiles_unkey(key)), lo, hi, step, inv, nbins);
      if (k >= 0) atomicAdd(&mine[k], 1u);
    });
    if (!ok) *flag = 1;
  }
  __syncthreads();
  for (int i = tid; i < cells; i += QNT_THREADS) {
    const unsigned c = hist1_s[i];
    if (c) atomicAdd(&h1[(size_t)fbase * (nbins + 2) + i], (qnt_u64)c);
  }
}

// ---- the 2-D kernel ----------------------------------------------------------------------------------------------------------------
// its dynamic LDS, for the kernel (the named pointers) and for its launch (`bytes`): nfeat features, nbins bins, tp pairs a tile
struct HistLds {
  long long* first;         // [HIST_WALKERS] the first row of each walker's window (-1: none)
  unsigned int* table;      // [tp][nbins * nbins] the tile's counters
  unsigned short* pair_i;   // [tp] the features of each pair of the tile
  unsigned short* pair_j;   // [tp]
  unsigned char* stage;     // [samples][nfeat] bin indices
  int samples;              // samples staged at a time
  size_t bytes;
  // the pairs of a tile: as many tables as HIST_TABLE_BYTES hold (1 at least: 128 * 128 counters are 64 KiB), HIST_PAIRS_MAX at most
  PTM_LDS_FN static int tile_pairs(int nbins, long long npairs, long long forced) {
    long long tp = HIST_TABLE_BYTES / ((long long)nbins * nbins * 4);
    if (tp > HIST_PAIRS_MAX) tp = HIST_PAIRS_MAX;
    if (forced > 0 && forced < tp) tp = forced;
    if (tp > npairs) tp = npairs;
    return tp < 1 ? 1 : (int)tp;
  }
  template <class C>
  PTM_LDS_FN void carve(C& c, int nfeat, int nbins, int tp) {
    samples = HIST_STAGE_BYTES / nfeat;
    c.take(first, "first", HIST_WALKERS);
    c.take(table, "table", tp * nbins * nbins);
    c.take(pair_i, "pair_i", (tp + 3) & ~3);
    c.take(pair_j, "pair_j", (tp + 3) & ~3);
    c.take(stage, "stage", HIST_STAGE_BYTES);
    bytes = c.size();
  }
  HistLds() = default;
  PTM_LDS_FN HistLds(void* base, int nfeat, int nbins, int tp) { LdsCarve c(base); carve(c, nfeat, nbins, tp); }
};

struct HistWalk {
  EssSrc src;
  const unsigned int* nhist;   // [walker] each chain's own count of add_state calls (null: src.steps for all)
  int W, nfeat, nbins;
  int nrows, rows_per_chunk;
  int tp, map;                 // pairs of a tile; HIST_MAP_*
  long long npairs;
};

// h2: [npairs][nbins * nbins] global counters.  2 <= nfeat <= HIST_STAGE_BYTES.
template <bool CHECK>
__global__ __launch_bounds__(HIST_THREADS) void histograms_2d_kernel(HistWalk q, const double* __restrict__ par, qnt_u64* __restrict__ h2, int* __restrict__ flag) {
  extern __shared__ unsigned char hist2_lds[];
  const HistLds L(hist2_lds, q.nfeat, q.nbins, q.tp);
  const int tid = (int)threadIdx.x, nfeat = q.nfeat, nbins = q.nbins, nb2 = nbins * nbins;
  const long long p0 = (long long)blockIdx.z * q.tp;
  const int tpc = (int)(q.npairs - p0 < q.tp ? q.npairs - p0 : q.tp), cells = tpc * nb2;
  const int w0 = (int)blockIdx.x * HIST_WALKERS, wc = q.W - w0 < HIST_WALKERS ? q.W - w0 : HIST_WALKERS;
  const long long r0 = (long long)blockIdx.y * q.rows_per_chunk;
  const int n = (int)(q.nrows - r0 < q.rows_per_chunk ? q.nrows - r0 : q.rows_per_chunk);
  for (int i = tid; i < cells; i += HIST_THREADS) L.table[i] = 0u;
  for (int i = tid; i < tpc; i += HIST_THREADS) {
    int a, b;
    histograms_pair(nfeat, p0 + i, &a, &b);
    L.pair_i[i] = (unsigned short)a;
    L.pair_j[i] = (unsigned short)b;
  }
  if (tid < wc) {
    // the window: ptm_rhat's rule (the caller has checked all of this: a lane never reads outside the ring)
    const long long steps = q.nhist ? (long long)q.nhist[w0 + tid] : (long long)q.src.steps;
    const long long newest = q.src.first_row + (steps - 1) / q.src.add_every, first = newest - q.nrows + 1;
    const bool bad = steps < 1 || first < q.src.first_row || q.nrows > q.src.cap || (!CHECK && newest >= q.src.cap);
    if (bad) *flag = 1;
    L.first[tid] = bad ? -1 : first;
  }
  __syncthreads();
  const long long total = (long long)n * wc;   // the samples of this workgroup: sample g is row g / wc of walker g % wc
  const int S = L.samples;
  for (long long g0 = 0; g0 < total; g0 += S) {
    const int sc = (int)(total - g0 < S ? total - g0 : S), elems = sc * nfeat;
    // stage: element e is feature e % nfeat of sample e / nfeat
    for (int e0 = tid; e0 < elems; e0 += HIST_THREADS * HIST_AHEAD) {
      double v[HIST_AHEAD];
      int feat[HIST_AHEAD];
      bool there[HIST_AHEAD];
#pragma unroll
      for (int a = 0; a < HIST_AHEAD; ++a) {
        const int e = e0 + a * HIST_THREADS;
        there[a] = e < elems;
        const int s = there[a] ? e / nfeat : 0;
        feat[a] = there[a] ? e - s * nfeat : 0;
        const long long g = g0 + s;
        const int row = (int)(g / wc), wl = (int)(g - (long long)row * wc);
        const long long first = L.first[wl];
        if (first < 0) there[a] = false;
        const long long slot = there[a] ? rhat_slot<CHECK>(q.src, CHECK ? q.src.meta + (w0 + wl) : nullptr, first + r0 + row) : 0;
        if (slot < 0) { *flag = 1; there[a] = false; }
        v[a] = there[a] ? q.src.x[slot * q.src.slot_stride + (long long)(w0 + wl) * q.src.series_stride + ess_pos(q.src, feat[a])] : 0.0;
      }
#pragma unroll
      for (int a = 0; a < HIST_AHEAD; ++a) {
        const int e = e0 + a * HIST_THREADS;
        if (e >= elems) continue;
        int k = HIST_OUTSIDE;
        if (there[a]) {
          const double* pf = par + (size_t)HIST_PAR * (size_t)feat[a];
          k = histograms_bin(v[a], pf[0], pf[1], pf[2], pf[3], nbins);
          if (k < 0 || k >= nbins) k = HIST_OUTSIDE;
        }
        L.stage[e] = (unsigned char)k;
      }
    }
    __syncthreads();
    // count: the (sample, pair) adds of the staged samples, dealt to the lanes
    const int items = sc * tpc;
    for (int it = tid; it < items; it += HIST_THREADS) {
      int s, p;
      if (q.map == HIST_MAP_PAIRS) { s = it / tpc; p = it - s * tpc; }
      else { p = it / sc; s = it - p * sc; }
      const unsigned char* row = L.stage + s * nfeat;
      const int ki = row[L.pair_i[p]], kj = row[L.pair_j[p]];
      if (ki != HIST_OUTSIDE && kj != HIST_OUTSIDE) atomicAdd(&L.table[p * nb2 + ki * nbins + kj], 1u);
    }
    __syncthreads();
  }
  for (int i = tid; i < cells; i += HIST_THREADS) {
    const unsigned c = L.table[i];
    if (c) atomicAdd(&h2[(size_t)p0 * nb2 + i], (qnt_u64)c);
  }
}

}  // namespace ptm
