// ptm_lds_layout.hpp -- the dynamic LDS of the kernels listed below: ONE description per kernel, read by the kernel (the named
// pointers), by its launch (`bytes`) and by tests/cxx/lds_layout_main.cc (every region's name, offset and length).  Plain C++: no HIP.
//
// A layout is a struct of pointers with one member template, carve(c, facts...), that takes its regions from a carve `c` in address
// order, and a constructor over a base pointer that runs it on an LdsCarve.  The kernel builds `const XLds L(lds_all, facts)` and uses
// L.name; the launch asks `XLds(nullptr, facts).bytes`.  The facts are exactly what the size depends on.  To change a kernel's LDS,
// edit its carve() here and nothing else; a new array is a member and a take.
//
// NOT here: the lanes kernels, the fused small-ladder kernel and the persistent ladder kernel (ptm_lanes_kernel.hpp, ptm_fused_kernel.hpp,
// ptm_ladder_kernel.hpp).  They still carve by hand, with lanes_lds_doubles and the functions of ptm_ladder_args.hpp as their byte counts:
// built from a layout, 36 builds of the ladder kernel (all spilling at the register limit) and one lanes build came out with other spill
// counts or another occupancy than before (the optimiser's output differed in the order of a few instructions), and a change of layout
// description is no reason to accept that.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PTM_LDS_FN __host__ __device__ __forceinline__
#else
#define PTM_LDS_FN inline
#endif

namespace ptm {

constexpr int BM_TABLE_DOUBLES = 512 + 2048;   // the Box-Muller table image (ptm_device_math.hpp: BM_TABLE)
constexpr int MVCAP = 256;            // rows one ladder can move per step on the register path (move_kernel)
constexpr int M64_P2_TILES = 40;      // 64-D matrix-core sweep: (row tile rt, step m) with m <= 4 rt + 3, at m64_p2_base(rt) + m
constexpr int M128_P2_TILES = 144;    // 128-D: at m128_p2_base(rt) + m
constexpr int M128_THREADS = 512;     // ... eight waves share the block's tables: two per SIMD at 256 registers each

// A bump carve: regions are taken one behind the other from a base pointer.  `bytes` is what the launch must allocate.
//   take(p, n)   p = n elements of p's type; the next region starts behind them (typed pointer arithmetic with an int count, one step
//                per region, as a hand-written chain of casts would be)
//   tail(live)   the takes from here on are an optional tail of the layout: they get their addresses either way (a kernel build that
//                never touches them costs nothing), and count towards `bytes` only when live.  Tails end a layout: live ones first,
//                and only slack may follow the last
//   slack(n)     n bytes behind everything, that nothing uses
//   reuse(p, b, e)  a carve that starts at the region p taken earlier, at offset b, for arrays that share the space of others whose life
//                is over.  e is the end of that space: the carve itself does not hold the takes to it (a kernel could do nothing about
//                it); the recording carve of tests/cxx/lds_layout_main.cc does, for every shape it lists
struct LdsCarve {
  unsigned char* cur;   // the next region (null: the launch asks without a base, sizes only)
  size_t off, bytes;
  bool live;
  PTM_LDS_FN explicit LdsCarve(void* b, size_t o = 0) : cur(static_cast<unsigned char*>(b)), off(o), bytes(o), live(true) {}
  template <class T>
  PTM_LDS_FN void take(T*& p, const char* /*name*/, int n) {
    p = reinterpret_cast<T*>(cur);
#if !defined(__HIP_DEVICE_COMPILE__)
    if (cur)
#endif
      cur = reinterpret_cast<unsigned char*>(p + n);
    off += (size_t)n * sizeof(T);
    if (live) bytes = off;
  }
  PTM_LDS_FN size_t at() const { return off; }       // the offset of the next take
  PTM_LDS_FN size_t size() const { return bytes; }
  PTM_LDS_FN void tail(bool on) { live = on; }
  PTM_LDS_FN void slack(const char* /*name*/, size_t n) { if (live) bytes += n; }
  template <class T>
  PTM_LDS_FN LdsCarve reuse(T* p, size_t begin, size_t /*end*/) const { LdsCarve r(p, begin); r.live = live; return r; }
};

// ---- decide_body (ptm_decide.hpp): decide_kernel, and the exchange phase of the fused small-ladder kernel
// Nt rungs, ms candidates per step, a window of WN rungs; evolve: evolving ladders, evb: ... with history / MAP tracking, cut: ... with a
// posterior-ordering cut (both only with evolve).  All offsets are multiples of 8.
struct DecideLds {
  double* llc;                   // [WN]  llike view of the touched rungs
  unsigned short* first;         // [Nt]  first pick of each rung value (NONE: not picked)
  int* cand;                     // [ms]  rung of the pick / -2 none or dropped
  uint32_t* ua;                  // [ms]  accept uniform of the pick (raw)
  int* cnt;                      // [4]   list length, move count, ambiguous trial seen, pries
  unsigned short *perm, *inv;    // [WN]  source rung of the row now at a rung, and its inverse
  unsigned short* list;          // [ms]  surviving picks that are ours
  unsigned short* midk;          // [ms]  (by pick) row the pick's lower rung held before a later pick on the pair below exchanged it again
  unsigned char* alive;          // [ms]  0 dropped, 1 survives and is ours, 2 survives, not ours
  unsigned char* accf;           // [ms]
  int* lmv;                      // [2][MVCAP]  the move list
  // evolving ladders only: gaps (in the end their local prefix sums), chunk totals / offsets, {normaliser, pries}, and the
  // surviving picks in PICK ORDER (position t): what the chain of dependent trials needs, laid out for one lane to stream
  double* gap;                   // [Nt]
  double* ct;                    // [2][(Nt + 31) / 32]
  double* ev;                    // [2]
  double* tlu;                   // [ms]  log of the pick's accept uniform
  double* tgap;                  // [ms]  the pick's gap (a pair is tried once: never pried before)
  double* tlla;                  // [ms]  llike of the lower rung (nothing earlier can change it)
  double* tllb;                  // [ms]  llike of the upper rung (an earlier pick above may change it)
  unsigned short* olist;         // [ms]  position -> pick
  unsigned short* opos;          // [ms]  pick -> position
  unsigned short* ti;            // [ms]  the pick's lower rung
  short* tdep;                   // [ms]  position of the (later) pick on the pair below, or -1
  unsigned char* tacc;           // [ms]  accepted
  // ... with history / MAP tracking on top (an add_state of the phase sees the temperature BETWEEN two pries of the step):
  double* p0;                    // [max(Nt, MVCAP)]  prefix sums of the step's first gaps
  double* gb;                    // [MVCAP] temperature for a HIST / MAP move: in p0's space (p0 is done by then)
  double* tS;                    // [ms]  sum of the gaps the pick saw (0: nothing pried yet)
  double* tdl;                   // [ms]  what the pick added to its gap
  double* bklo;                  // [ms]  (by pick) temperature of the pick's lower rung then
  double* tbl;                   // [ms]  stored temperature of the pick's lower rung (asked for with the other operands:
  double* tbh;                   // [ms]  ... and of its upper rung     a trip to memory off the phase's critical path)
  // ... with a posterior-ordering cut (the carve above is then taken as with history): the current llike and lprior of EVERY rung,
  // exchanged as the picks are decided
  double *llv, *lpv;             // [Nt]
  bool aliased;
  size_t bytes;

  // perm, inv and the move list are not needed before the trials of an evolving ladder are over, whose operand arrays (tlu .. tllb) are
  // dead by then: they share that space when it is big enough -- 6 KB less per block, a fifth block per CU for 1024-rung ladders
  PTM_LDS_FN static bool alias_rule(int ms, int WN, bool evolve) {
    return evolve && (size_t)2 * ((WN + 3) & ~3) * 2 + (size_t)2 * MVCAP * 4 <= (size_t)4 * ((ms + 3) & ~3) * 8;
  }
  template <class C>
  PTM_LDS_FN void carve(C& c, int Nt, int ms, int WN, bool evolve, bool evb, bool cut) {
    const int WNp = (WN + 3) & ~3, msp = (ms + 3) & ~3, ms2 = (ms + 1) & ~1, ms8 = (ms + 7) & ~7;
    aliased = alias_rule(ms, WN, evolve);
    c.take(llc, "llc", WN);
    c.take(first, "first", (Nt + 3) & ~3);
    c.take(cand, "cand", ms2);
    c.take(ua, "ua", ms2);
    c.take(cnt, "cnt", 4);
    if (!aliased) { c.take(perm, "perm", WNp); c.take(inv, "inv", WNp); }
    c.take(list, "list", msp);
    c.take(midk, "midk", msp);
    c.take(alive, "alive", ms8);
    c.take(accf, "accf", ms8);
    if (!aliased) c.take(lmv, "lmv", 2 * MVCAP);
    c.tail(evolve);
    c.take(gap, "gap", Nt);
    c.take(ct, "ct", 2 * ((Nt + 31) / 32));
    c.take(ev, "ev", 2);
    const size_t operands = c.at();
    c.take(tlu, "tlu", msp);
    c.take(tgap, "tgap", msp);
    c.take(tlla, "tlla", msp);
    c.take(tllb, "tllb", msp);
    if (aliased) {
      C o = c.reuse(tlu, operands, c.at());
      o.take(inv, "inv", WNp); o.take(perm, "perm", WNp); o.take(lmv, "lmv", 2 * MVCAP);
    }
    c.take(olist, "olist", msp);
    c.take(opos, "opos", msp);
    c.take(ti, "ti", msp);
    c.take(tdep, "tdep", msp);
    c.take(tacc, "tacc", ms8);
    c.tail(evolve && (evb || cut));
    const size_t p0_at = c.at();
    c.take(p0, "p0", Nt > MVCAP ? Nt : MVCAP);
    { C o = c.reuse(p0, p0_at, c.at()); o.take(gb, "gb", MVCAP); }
    c.take(tS, "tS", msp);
    c.take(tdl, "tdl", msp);
    c.take(bklo, "bklo", msp);
    c.take(tbl, "tbl", msp);
    c.take(tbh, "tbh", msp);
    c.tail(evolve && cut);
    c.take(llv, "llv", Nt);
    c.take(lpv, "lpv", Nt);
    c.tail(true);
    c.slack("slack", 32);
    bytes = c.size();
  }
  DecideLds() = default;
  PTM_LDS_FN DecideLds(void* base, int Nt, int ms, int WN, bool evolve, bool evb, bool cut) { LdsCarve c(base); carve(c, Nt, ms, WN, evolve, evb, cut); }
};

// the rungs' tile prefix of a compacted launch (the compacted 32-D sweep and the box pre-pass): the scan's chunk totals, and their sum
constexpr int TILE_SCAN_INTS = 257, TILE_SCAN_SLACK = 3 * sizeof(int);

// ---- sweep_mfma32_kernel (ptm_mfma_kernel.hpp).  gen: a general build (GEN > 0); compacted: a launch over nrung rungs' lists
struct Mfma32Lds {
  double* bm;              // [2560] Box-Muller tables
  double* ptile;           // [12][64] precision tiles: (row tile 1, step m) at m*64, m = 0..7; (row tile 0, step m) at (8+m)*64, m = 0..3
  double* lbox;            // [64] prior box
  double* red;             // [4][128] reduction slots per wave
  // gen: per-dimension tables of the state space and the prior, natural index
  double* gtab = nullptr;  // bmin | bmax | plo | phi | pcoef | mean, 32 each
  int* gint = nullptr;     // blo | bhi | ptype, 32 each
  double* red2 = nullptr;  // [4][128] the prior's partial products, per wave
  double* ebox = nullptr;  // [64] all boundaries open or `limit` (the usual case): enforcing is a box test -- lower | upper limits in row layout
  // compacted: the launch's rungs, their listed-walker counts as an inclusive prefix of 256-walker tiles
  int* tpre = nullptr;     // [nrung]
  int* tsum = nullptr;     // [257] chunk totals -> exclusive offsets, and the number of tiles
  size_t bytes;
  template <class C>
  PTM_LDS_FN void carve(C& c, bool gen, bool compacted, int nrung) {
    c.take(bm, "bm", BM_TABLE_DOUBLES);
    c.take(ptile, "ptile", 12 * 64);
    c.take(lbox, "lbox", 64);
    c.take(red, "red", 4 * 128);
    if (gen) {
      c.take(gtab, "gtab", 6 * 32);
      c.take(gint, "gint", 3 * 32);
      c.take(red2, "red2", 4 * 128);
      c.take(ebox, "ebox", 64);
    }
    if (compacted) {
      c.take(tpre, "tpre", nrung);
      c.take(tsum, "tsum", TILE_SCAN_INTS);
      c.slack("slack", TILE_SCAN_SLACK);
    }
    bytes = c.size();
  }
  Mfma32Lds() = default;
  PTM_LDS_FN Mfma32Lds(void* base, bool gen, bool compacted, int nrung) { LdsCarve c(base); carve(c, gen, compacted, nrung); }
};

// ---- box_prefilter_kernel / box_prefilter_f32_kernel (ptm_box_prefilter.hpp): a launch over nrung rungs; tables: the pass draws from
// the Box-Muller tables (the double-precision one)
struct BoxPreLds {
  double* bm = nullptr;   // Box-Muller tables
  double* lbox;   // [64] prior box
  int* tpre;      // [nrung] inclusive prefix of the rungs' 256-walker tiles
  int* pcn;       // [nrung] the rungs' list lengths
  int* tsum;      // [257]
  size_t bytes;
  template <class C>
  PTM_LDS_FN void carve(C& c, bool tables, int nrung) {
    if (tables) c.take(bm, "bm", BM_TABLE_DOUBLES);
    c.take(lbox, "lbox", 64);
    c.take(tpre, "tpre", nrung);
    c.take(pcn, "pcn", nrung);
    c.take(tsum, "tsum", TILE_SCAN_INTS);
    c.slack("slack", TILE_SCAN_SLACK);
    bytes = c.size();
  }
  BoxPreLds() = default;
  PTM_LDS_FN BoxPreLds(void* base, bool tables, int nrung) { LdsCarve c(base); carve(c, tables, nrung); }
};

// ---- sweep_kernel (ptm_kernels.hpp): the 20 KB of Box-Muller tables every variant stages; the builds whose waves share a rung and
// whose factor is not diagonal (staged) keep one copy of the rung's factor per wave too (4 waves per block)
struct GeneralLds {
  double* bm;
  double* fac = nullptr;   // [4][prop_stride]
  size_t bytes;
  template <class C>
  PTM_LDS_FN void carve(C& c, bool staged, int prop_stride) {
    c.take(bm, "bm", BM_TABLE_DOUBLES);
    if (staged) c.take(fac, "fac", 4 * prop_stride);
    bytes = c.size();
  }
  GeneralLds() = default;
  PTM_LDS_FN GeneralLds(void* base, bool staged, int prop_stride) { LdsCarve c(base); carve(c, staged, prop_stride); }
};

// ---- sweep_mfma64_kernel / sweep_mfma128_kernel: D dimensions, `waves` waves share the block's tables
template <int D, int TILES, int WAVES>
struct MfmaWideLds {
  double* bm;      // Box-Muller tables
  double* ptile;   // [TILES][64] precision tiles
  double* lbox;    // [2][D] prior box lo | hi (row layout)
  double* red;     // [WAVES][64] reduction slots per wave
  double* lebox;   // [2][D] boundary::enforce for open / limit sides (states.cc:53-55) as a box, row layout
  size_t bytes;
  template <class C>
  PTM_LDS_FN void carve(C& c) {
    c.take(bm, "bm", BM_TABLE_DOUBLES);
    c.take(ptile, "ptile", TILES * 64);
    c.take(lbox, "lbox", 2 * D);
    c.take(red, "red", WAVES * 64);
    c.take(lebox, "lebox", 2 * D);
    bytes = c.size();
  }
  MfmaWideLds() = default;
  PTM_LDS_FN explicit MfmaWideLds(void* base) { LdsCarve c(base); carve(c); }
};
typedef MfmaWideLds<64, M64_P2_TILES, 4> Mfma64Lds;
typedef MfmaWideLds<128, M128_P2_TILES, M128_THREADS / 64> Mfma128Lds;   // (97 KB: one block per CU)

}  // namespace ptm
