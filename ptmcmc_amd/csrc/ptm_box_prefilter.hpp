// ptm_box_prefilter.hpp -- a pass between partition_kernel and the compacted lean sweep (ptm_mfma_kernel.hpp) that settles the chains
// whose proposal has left the uniform prior box in its first 16 dimensions already; included by ptm_engine.hip only.
//
// On the hot rungs of a long ladder most proposals land outside the box and are rejected whatever their likelihood is, yet in the
// sweep each of them pays for all 32 normals, both matrix products and the Metropolis test.  With a lower-triangular factor rows
// 0..15 of T Z take columns 0..15 only, and those are the normals of each lane's FIRST Philox block (hb == 0, block 1 + q): the
// first 16 coordinates of a proposal cost 4 of the sweep's 9 Philox blocks per lane and tile, half of its Box-Muller work and 16 of
// its 96 MFMAs.  This kernel draws exactly that -- the same stream, the same tables in LDS, the same accumulation order as the
// sweep, so x'[0..15] is bit for bit the sweep's -- and box-tests it.  A chain found outside does what the sweep would have done
// with it (chain.cc:973-1019 with newlprior = -inf): ntries += 1 and nothing else.  Everybody else is appended to the sweep's own
// list of the rung, and the sweep does for them what it always did, the first half's draw included.
// A chain whose CURRENT log-posterior is not finite is never settled here: its logH is NaN and the reference accepts the move
// ("NaN stays accepted", ptm_mfma_kernel.hpp stage 5), wherever the proposal lands.
//
// Lane roles are the sweep's: one wave = 64 listed walkers of one rung, lane l = 16q + j works in the matrix product for chains
// 16g + j, g = 0..3, on dimensions q + 4m, m < 4 (the 16-byte pieces 0..7 of the row), and owns chain l for the per-chain work.
// The grid is persistent like the sweep's (the 20 KB of Box-Muller tables are staged once per resident block), and the two
// counters (chains seen, chains settled) are summed per wave over all its tiles: two atomics per wave and launch.
#pragma once
#include "ptm_kernels.hpp"

namespace ptm {

struct BoxPre {
  int W, Nt, r0, w_off;
  int rung0, nrung;            // the launch's local rungs
  int labelled;                // a list entry is walker | slot << 16 (row labels), the row sits at rung slot `slot`
  uint64_t seed, step;
  const double* x;             // [Nc][32] rows
  const double *ll, *lp;       // [Nc]
  const double* beta;          // [Nt] global
  const double* prop_tiles;    // [nloc][16][64]
  const double* box_row;       // [2][32]
  int* ntries;                 // [Nc]
  const int *pidx, *pcnt;      // this pass's lists (partition_kernel, flagged rungs): pidx[rl * W ..), pcnt[rl] entries
  int *cidx, *ccnt;            // the sweep's lists: the survivors are appended
  unsigned long long* counts;  // {chains seen, chains settled}, accumulated
};

typedef double bp_d4 __attribute__((ext_vector_type(4)));
typedef double bp_d2 __attribute__((ext_vector_type(2)));

// dynamic LDS of a launch over nrung rungs: tables | box | the rungs' tile prefix and the scan's chunk totals
inline size_t box_prefilter_lds(int nrung) { return (size_t)(BM_TABLE_DOUBLES + 64) * sizeof(double) + ((size_t)nrung + 260) * sizeof(int); }

__global__ __launch_bounds__(256) void box_prefilter_kernel(const BoxPre p) {
  extern __shared__ __attribute__((aligned(16))) double bp_lds[];
  double* lbox = bp_lds + BM_TABLE_DOUBLES;
  int* tpre = reinterpret_cast<int*>(lbox + 64);   // [nrung] inclusive prefix of the rungs' 256-walker tiles
  const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, q = l >> 4, j = l & 15;
#pragma unroll
  for (int t = 0; t < BM_TABLE_DOUBLES / 512; ++t)
    reinterpret_cast<bm_d2*>(bp_lds)[threadIdx.x + 256 * t] = reinterpret_cast<const bm_d2*>(BM_TABLE)[threadIdx.x + 256 * t];
  if (threadIdx.x < 64) lbox[threadIdx.x] = p.box_row[threadIdx.x];
  // inclusive scan of ceil(count / 256) over the rungs, as in the compacted sweep
  const int nrung = p.nrung, per = (nrung + 255) / 256;
  int loc = 0;
  for (int k = 0; k < per; ++k) {
    const int r = threadIdx.x * per + k;
    if (r < nrung) { loc += (p.pcnt[p.rung0 + r] + 255) >> 8; tpre[r] = loc; }
  }
  int* tsum = tpre + nrung;   // [257]
  tsum[threadIdx.x] = loc;
  __syncthreads();
  if (threadIdx.x == 0) { int run = 0; for (int t = 0; t < 256; ++t) { const int v = tsum[t]; tsum[t] = run; run += v; } tsum[256] = run; }
  __syncthreads();
  const int off = tsum[threadIdx.x];
  for (int k = 0; k < per; ++k) {
    const int r = threadIdx.x * per + k;
    if (r < nrung) tpre[r] += off;
  }
  __syncthreads();
  const int ntiles = tsum[256];
  const bp_d2* box = reinterpret_cast<const bp_d2*>(lbox) + q;   // lo piece t at 4t, hi piece t at 16 + 4t (row layout)
  const int wmask = p.labelled ? 0xFFFF : -1;
  unsigned int seen = 0, settled = 0;   // (wave-uniform)
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int lo = 0, hi = nrung - 1;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (tpre[mid] > tile) hi = mid; else lo = mid + 1; }
    const int r = __builtin_amdgcn_readfirstlane(lo);
    const int kb = tile - (r ? tpre[r - 1] : 0);
    const int rl = p.rung0 + r, rg = p.r0 + rl;
    const int start = (kb * 4 + wave) * 64, cnt = p.pcnt[rl];
    if (start >= cnt) continue;   // (only wave-level work below)
    const int nact = cnt - start < 64 ? cnt - start : 64;
    const size_t lbase = (size_t)rl * p.W;
    // lanes past the list shadow its last entry and write nothing
    const int mine = p.pidx[lbase + start + (l < nact ? l : nact - 1)];
    const int c = (int)lbase + (mine & wmask);
    const double ll = p.ll[c], lp = p.lp[c];
    const double beta = as_c(p.beta)[rg];
    const double* timg = p.prop_tiles + (size_t)rl * (16 * 64) + l;
    double ta[4];
#pragma unroll
    for (int sl = 0; sl < 4; ++sl) ta[sl] = timg[((0 * 4 + sl) * 2 + 0) * 64];
    const bp_d2 lo0 = box[0], lo1 = box[4], hi0 = box[16], hi1 = box[20];
    bp_d2 v0[4], v1[4];
    int wk[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int e = __shfl(mine, 16 * g + j, 64);
      const int slot = p.labelled ? (int)((unsigned int)e >> 16) : rl;
      wk[g] = e & wmask;
      const bp_d2* rp = reinterpret_cast<const bp_d2*>(p.x + ((size_t)slot * p.W + wk[g]) * 32) + q;
      v0[g] = rp[0];
      v1[g] = rp[4];
    }
    uint64_t inbox = 0;   // bit 16 g + j: chain (g, j) is inside the box in dimensions 0..15
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const uint32_t stream = (uint32_t)(wk[g] + p.w_off) * (uint32_t)p.Nt + (uint32_t)rg;
      const u32x4 o = draw_block(p.seed, TAG_MH, stream, p.step, (uint32_t)(1 + q));
      double z[4];
      boxmuller(o.v0, o.v1, (const double*)bp_lds, z[0], z[1]);
      boxmuller(o.v2, o.v3, (const double*)bp_lds, z[2], z[3]);
      bp_d4 acc = bp_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int sl = 0; sl < 4; ++sl) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ta[sl], z[sl], acc, 0, 0, 0);
      const double x0 = v0[g].x + acc[0], x1 = v0[g].y + acc[1], x2 = v1[g].x + acc[2], x3 = v1[g].y + acc[3];
      const bool ok = !(x0 < lo0.x) & !(x0 > hi0.x) & !(x1 < lo0.y) & !(x1 > hi0.y) & !(x2 < lo1.x) & !(x2 > hi1.x) & !(x3 < lo1.y) & !(x3 > hi1.y);
      uint64_t b = __builtin_amdgcn_ballot_w64(ok);
      b &= b >> 32;
      b &= b >> 16;   // bit jj: all four lanes (q, jj) of chain (g, jj) are inside
      inbox |= (b & 0xFFFFull) << (16 * g);
    }
    // chain l of the wave: the sweep's cur_lpost, rounded as the sweep rounds it
    const double cur_lpost = lp + beta * ll;
    const bool live = l < nact;
    const bool finite = __builtin_fabs(cur_lpost) < __builtin_inf();   // (false for NaN)
    const bool settle = live && finite && ((inbox >> l) & 1ull) == 0;
    if (settle) p.ntries[c] += 1;
    const bool keep = live && !settle;
    const uint64_t kbits = __builtin_amdgcn_ballot_w64(keep);
    const int nk = __builtin_popcountll(kbits);
    int base = 0;
    if (l == 0 && nk) base = atomicAdd(&p.ccnt[rl], nk);
    base = __builtin_amdgcn_readfirstlane(base);
    if (keep) p.cidx[lbase + base + __builtin_popcountll(kbits & ((1ull << l) - 1ull))] = mine;
    seen += (unsigned int)nact;
    settled += (unsigned int)(nact - nk);
  }
  if (l == 0 && seen) {
    atomicAdd(p.counts, (unsigned long long)seen);
    if (settled) atomicAdd(p.counts + 1, (unsigned long long)settled);
  }
}

}  // namespace ptm
