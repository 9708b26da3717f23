// ptm_box_prefilter.hpp -- a pass between partition_kernel and the compacted lean sweep (ptm_mfma_kernel.hpp) that settles the chains
// whose proposal has left the uniform prior box in its first 16 dimensions already; included by ptm_engine.hip only.
//
// On the hot rungs of a long ladder most proposals land outside the box and are rejected whatever their likelihood is, yet in the
// sweep each of them pays for all 32 normals, both matrix products and the Metropolis test.  With a lower-triangular factor rows
// 0..15 of T Z take columns 0..15 only, and those are the normals of each lane's FIRST Philox block (hb == 0, block 1 + q): the
// first 16 coordinates of a proposal cost 4 of the sweep's 9 Philox blocks per lane and tile, half of its Box-Muller work and 16 of
// its 96 MFMAs.  This pass draws exactly that from the sweep's stream and box-tests it.  A chain found outside does what the sweep
// would have done with it (chain.cc:973-1019 with newlprior = -inf): ntries += 1 and nothing else.  Everybody else is appended to the
// sweep's own list of the rung, and the sweep does for them what it always did, the first half's draw included.
// A chain whose CURRENT log-posterior is not finite is never settled here: its logH is NaN and the reference accepts the move
// ("NaN stays accepted", ptm_mfma_kernel.hpp stage 5), wherever the proposal lands.
//
// There is ONE body, box_prefilter_body, and two kernels that call it with their arithmetic (below: BpExact, BpF32): what a lane draws
// and multiplies, and which faces it tests against.  Everything else exists once.
//
// Lane roles are the sweep's: one wave = 64 listed walkers of one rung, lane l = 16q + j works in the matrix product for chains
// 16g + j, g = 0..3, on dimensions q + 4m, m < 4 (the 16-byte pieces 0..7 of the row), and owns chain l for the per-chain work.
// The grid is persistent like the sweep's, and the two counters (chains seen, chains settled) are summed per wave over all its
// tiles: two atomics per wave and launch.
//
// The tile loop is a pipeline over the block's tiles t, t + G, t + 2G, ... (G blocks): a tile's work is a chain of dependent trips to
// memory -- list length, list entry, the rows / ll / lp / factor tiles it names, the counter's old value, the sweep list's old length
// -- and a wave that makes them one after the other stands idle most of the time.  So: the list lengths sit in LDS beside the tile
// prefix (the prologue reads them anyway); the list entry is asked for one tile before its draw; ntries is an atomic add nobody
// waits for; and the append to the sweep's list asks for its place at the end of tile t and stores the survivors at the end of the
// wave's next tile (after the loop for the last one).  The order of a sweep list is arbitrary: any order gives the same chains.
#pragma once
#include "ptm_kernels.hpp"
#include "ptm_sweep_plan.hpp"

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

struct BoxPreF32 {
  BoxPre b;
  const float* margin;         // [nloc][4][4] the rungs' margins, rounded up to float: lane group q's four dimensions q + 4 i side by side
};

typedef double bp_d4 __attribute__((ext_vector_type(4)));
typedef double bp_d2 __attribute__((ext_vector_type(2)));
typedef float bp_f4 __attribute__((ext_vector_type(4)));

// scheduling fence (ptm_mfma_kernel.hpp: PTM_STAGE): the loads asked ahead stay in front of the arithmetic they are to hide behind
#define PTM_BP_STAGE() __builtin_amdgcn_sched_barrier(0)
// The memory counter retires in order, and the compiler can only wait for "everything up to" a load.  So the one wait of a tile
// stands where everything outstanding is old: behind the draw -- the loads asked at the tile's top and the previous tile's append
// have had the whole draw to arrive -- and in front of this tile's own atomics, which nobody waits for before the same place of
// the next tile.  (s_waitcnt vmcnt(0), the other counters untouched.)
#define PTM_BP_ARRIVED() __builtin_amdgcn_s_waitcnt(0x0F70)

// what a tile reads through its list entries: the row pieces 0..7 of the wave's four groups, chain l's ll / lp, the rung's beta and
// the four factor operands of the rt == 0 accumulator
struct BpRows {
  bp_d2 v0[4], v1[4];
  double ll, lp, beta, ta[4];
};

// ---- the arithmetic of a pass: the policy A of box_prefilter_body --------------------------------------------------------------
//   EXACT                the sweep's own arithmetic, from the Box-Muller tables: the body stages their 20 KB in LDS, once per
//                        resident block.  Otherwise single precision behind a margin, and no tables
//   Rows                 BpRows, and whatever else the pass reads per tile
//   Factor               the tile's factor operands as the product takes them, where that is not as they are loaded
//   factor_lane(l,q,j)   whose factor operand lane l = 16 q + j takes
//   load_more(R, rl, q)  asks for the rest of Rows, between the factor operands and the rows
// The per-group step itself -- four Philox words to four normals, the product, the faces -- stands in the body under `if constexpr
// (A::EXACT)`, once per arithmetic: as a member of the policy the single-precision step came out of the compiler in another order
// (the conversion of the factor operands, which only the tile's first group makes, moved in front of the draw it is to hide behind).

// the sweep's arithmetic: the same tables, the same accumulation order, so x'[0..15] is bit for bit the sweep's and the box test is
// exact (PTM_BOX_PREFILTER_EXACT=1; the yardstick of the pass below, and a fallback)
struct BpExact {
  static constexpr bool EXACT = true;
  typedef BpRows Rows;
  struct Factor {};
  __device__ __forceinline__ static int factor_lane(int l, int, int) { return l; }
  __device__ __forceinline__ void load_more(Rows&, int, int) const {}
};

// The same pass from single-precision normals, the default.  Nothing downstream reads x'[0..15]: a settled chain gets ntries += 1, a kept
// one is drawn again from scratch by the sweep.  The pass answers one question -- is this proposal CERTAINLY outside the box in
// dimensions 0..15 -- and that needs the normals to three digits.  So: the same Philox stream, boxmuller_f32 (ptm_device_math.hpp: no
// table, no f64), T Z on v_mfma_f32_16x16x4_f32 from factor operands converted once per tile, x' = x + double(acc) in f64, and a chain
// is settled only where some owned dimension has x' < lo - m or x' > hi + m, m the rung's margin (ptm_sweep_plan.hpp:
// prefilter_margins, the error budget is written down there).  A proposal the margin leaves in doubt, and a NaN anywhere, goes to the
// sweep: the chains are bit for bit what they are with BpExact, which settles a superset.
// The margins are the rung's, made on the host (the engine's prefilter_flags), rounded up to float and read per tile beside beta and the
// factor operands, 16 bytes per lane; each group widens them and pushes the box out again -- 4 conversions and 8 additions per group.
// That is what fits four waves per SIMD: 127 registers.  Double-precision margins, or the pushed box kept from group to group, take
// 137, nine of them spilled at four waves; the pushed box read per tile from a host-made image 151.
// The f32 instruction's accumulator holds rows 4 q + i of its A operand where the f64 one holds rows q + 4 i, and the stored rows, the box
// and the margins are laid out for the latter (row_pos): lane 16 k + i takes the factor operand of lane 16 k + (i >> 2) + 4 (i & 3), which
// puts row q + 4 i of T at row 4 q + i of A.
struct BpF32 {
  const float* margin;
  static constexpr bool EXACT = false;
  struct Rows : BpRows { bp_f4 mg; };
  struct Factor { float ta[4]; };
  __device__ __forceinline__ static int factor_lane(int, int q, int j) { return 16 * q + (j >> 2) + 4 * (j & 3); }
  __device__ __forceinline__ void load_more(Rows& R, int rl, int q) const { R.mg = reinterpret_cast<const bp_f4*>(margin + (size_t)rl * PREFILTER_DIMS)[q]; }
};

template <class A>
__device__ __forceinline__ void box_prefilter_body(const BoxPre p, const A a) {
  extern __shared__ __attribute__((aligned(16))) double bp_lds[];
  typedef typename A::Rows Rows;
  const int nrung = p.nrung;
  const BoxPreLds L(bp_lds, A::EXACT, nrung);
  const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, q = l >> 4, j = l & 15;
  if constexpr (A::EXACT) {
#pragma unroll
    for (int t = 0; t < BM_TABLE_DOUBLES / 512; ++t)
      reinterpret_cast<bm_d2*>(L.bm)[threadIdx.x + 256 * t] = reinterpret_cast<const bm_d2*>(BM_TABLE)[threadIdx.x + 256 * t];
  }
  if (threadIdx.x < 64) L.lbox[threadIdx.x] = p.box_row[threadIdx.x];
  const int ntiles = tile_prefix_scan<true>(p.pcnt, p.rung0, nrung, L.tpre, L.tsum, L.pcn);   // (the counts stay in LDS for the tile loop)
  const bp_d2* box = reinterpret_cast<const bp_d2*>(L.lbox) + q;   // lo piece t at 4t, hi piece t at 16 + 4t (row layout)
  const int wmask = p.labelled ? 0xFFFF : -1;
  const int G = (int)gridDim.x;
  const int lt = A::factor_lane(l, q, j);

  // the wave's slice of a tile (wave-uniform; nact == 0: nothing to load, nothing to do) ...
  auto slice_of = [&](int tile) {
    PrefilterSlice s = prefilter_slice(L.tpre, L.pcn, nrung, ntiles, tile, wave);
    s.r = __builtin_amdgcn_readfirstlane(s.r);
    s.start = __builtin_amdgcn_readfirstlane(s.start);
    s.nact = __builtin_amdgcn_readfirstlane(s.nact);
    return s;
  };
  // ... its list entries: lanes past the list shadow its last entry and write nothing
  auto load_entry = [&](const PrefilterSlice& s) {
    if (s.nact == 0) return 0;
    return p.pidx[(size_t)(p.rung0 + s.r) * p.W + s.start + (l < s.nact ? l : s.nact - 1)];
  };
  // ... and what the entries name
  auto load_rows = [&](const PrefilterSlice& s, int mine, Rows& R) {
    if (s.nact == 0) return;
    const int rl = p.rung0 + s.r;
    const int c = (int)((size_t)rl * p.W) + (mine & wmask);
    R.ll = p.ll[c]; R.lp = p.lp[c];
    R.beta = as_c(p.beta)[p.r0 + rl];
    const double* timg = p.prop_tiles + (size_t)rl * (16 * 64) + lt;
#pragma unroll
    for (int sl = 0; sl < 4; ++sl) R.ta[sl] = timg[((0 * 4 + sl) * 2 + 0) * 64];
    a.load_more(R, rl, q);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int e = __shfl(mine, 16 * g + j, 64);
      const int slot = p.labelled ? (int)((unsigned int)e >> 16) : rl;
      const bp_d2* rp = reinterpret_cast<const bp_d2*>(p.x + ((size_t)slot * p.W + (e & wmask)) * 32) + q;
      R.v0[g] = rp[0];
      R.v1[g] = rp[4];
    }
  };

  PrefilterSlice s = slice_of((int)blockIdx.x);   // the slice and the entries of the tile at hand: asked for one tile ahead
  int mine = load_entry(s);
  Rows T = {};
  // the append whose place in the sweep's list is still on its way: survivors pbits of the entries pmine, rung list at plbase
  uint64_t pbits = 0;
  int pmine = 0, pbase = 0;
  size_t plbase = 0;
  auto flush = [&]() {
    if (pbits == 0) return;
    const int base = __builtin_amdgcn_readfirstlane(pbase);
    if ((pbits >> l) & 1ull) p.cidx[plbase + base + __builtin_popcountll(pbits & ((1ull << l) - 1ull))] = pmine;
    pbits = 0;
  };
  PTM_BP_ARRIVED();   // (the loop starts with nothing on its way but what it asks for itself)
  unsigned int seen = 0, settled = 0;   // (wave-uniform)
  for (int tile = blockIdx.x; tile < ntiles; tile += G) {
    // ask ahead: a tile past the end and an empty slice load nothing
    const PrefilterSlice sn = slice_of(tile + G);
    const int mn = load_entry(sn);
    load_rows(s, mine, T);
    PTM_BP_STAGE();
    const int nact = s.nact;   // (wave-uniform: only wave-level branches below)
    const int rl = p.rung0 + s.r, rg = p.r0 + rl;
    const size_t lbase = (size_t)rl * p.W;
    uint64_t inbox = 0;   // bit 16 g + j: chain (g, j) is not found outside the box in dimensions 0..15
    if (nact) {
      bp_d2 lo0, lo1, hi0, hi1;
      if constexpr (A::EXACT) { lo0 = box[0]; lo1 = box[4]; hi0 = box[16]; hi1 = box[20]; }   // the faces as they are stored
      typename A::Factor fac;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int wk = __shfl(mine, 16 * g + j, 64) & wmask;
        const uint32_t stream = (uint32_t)(wk + p.w_off) * (uint32_t)p.Nt + (uint32_t)rg;
        const u32x4 o = draw_block(p.seed, TAG_MH, stream, p.step, (uint32_t)(1 + q));
        double x0, x1, x2, x3;   // the lane's four coordinates of the group's proposals
        if constexpr (A::EXACT) {
          double z[4];
          boxmuller(o.v0, o.v1, L.bm, z[0], z[1]);
          boxmuller(o.v2, o.v3, L.bm, z[2], z[3]);
          bp_d4 acc = bp_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int k = 0; k < 4; ++k) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(T.ta[k], z[k], acc, 0, 0, 0);
          x0 = T.v0[g].x + acc[0]; x1 = T.v0[g].y + acc[1]; x2 = T.v1[g].x + acc[2]; x3 = T.v1[g].y + acc[3];
        } else {
          float z[4];
          boxmuller_f32(o.v0, o.v1, z[0], z[1]);
          boxmuller_f32(o.v2, o.v3, z[2], z[3]);
          if (g == 0) {   // (the rung is the wave's: once per tile, behind the first draw the loads hide behind)
#pragma unroll
            for (int k = 0; k < 4; ++k) fac.ta[k] = (float)T.ta[k];
          }
          // the faces pushed out by the margin
          const double m0 = (double)T.mg[0], m1 = (double)T.mg[1], m2 = (double)T.mg[2], m3 = (double)T.mg[3];
          lo0 = box[0] - bp_d2{m0, m1}; lo1 = box[4] - bp_d2{m2, m3}; hi0 = box[16] + bp_d2{m0, m1}; hi1 = box[20] + bp_d2{m2, m3};
          bp_f4 acc = bp_f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int k = 0; k < 4; ++k) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fac.ta[k], z[k], acc, 0, 0, 0);
          x0 = T.v0[g].x + (double)acc[0]; x1 = T.v0[g].y + (double)acc[1]; x2 = T.v1[g].x + (double)acc[2]; x3 = T.v1[g].y + (double)acc[3];
        }
        // out: a comparison with a NaN on either side is false, so a NaN in the row, the product or the faces keeps the chain
        const bool out = (x0 < lo0.x) | (x0 > hi0.x) | (x1 < lo0.y) | (x1 > hi0.y) | (x2 < lo1.x) | (x2 > hi1.x) | (x3 < lo1.y) | (x3 > hi1.y);
        uint64_t b = __builtin_amdgcn_ballot_w64(!out);
        b &= b >> 32;
        b &= b >> 16;   // bit jj: none of the four lanes (q, jj) of chain (g, jj) found it outside
        inbox |= (b & 0xFFFFull) << (16 * g);
      }
    }
    PTM_BP_STAGE();
    PTM_BP_ARRIVED();
    if (nact) {
      // chain l of the wave: the sweep's cur_lpost, rounded as the sweep rounds it
      const int c = (int)lbase + (mine & wmask);
      const double cur_lpost = T.lp + T.beta * T.ll;
      const bool live = l < nact;
      const bool finite = __builtin_fabs(cur_lpost) < __builtin_inf();   // (false for NaN)
      const bool settle = live && finite && ((inbox >> l) & 1ull) == 0;
      const bool keep = live && !settle;
      const uint64_t kbits = __builtin_amdgcn_ballot_w64(keep);
      const int nk = __builtin_popcountll(kbits);
      flush();   // the wave's previous append: its place has arrived
      // (this kernel's only writer of the chain's counter: the add needs no return and no wait)
      if (settle) (void)__hip_atomic_fetch_add(&p.ntries[c], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (nk) {
        pbits = kbits; pmine = mine; plbase = lbase;
        // the rung through a lane-wise move: on a wave-uniform address the compiler rewrites the add for the whole wave and
        // broadcasts its return on the spot, which is the wait this append is built to avoid
        const int rlv = __builtin_amdgcn_mov_dpp(rl, 0xE4, 0xF, 0xF, true);
        if (l == 0) pbase = atomicAdd(&p.ccnt[rlv], nk);
      }
      seen += (unsigned int)nact;
      settled += (unsigned int)(nact - nk);
    }
    s = sn; mine = mn;
  }
  flush();
  if (l == 0 && seen) {
    atomicAdd(p.counts, (unsigned long long)seen);
    if (settled) atomicAdd(p.counts + 1, (unsigned long long)settled);
  }
}

__global__ __launch_bounds__(256, 4) void box_prefilter_kernel(const BoxPre p) { box_prefilter_body(p, BpExact{}); }
__global__ __launch_bounds__(256, 4) void box_prefilter_f32_kernel(const BoxPreF32 pf) { box_prefilter_body(pf.b, BpF32{pf.margin}); }

}  // namespace ptm
