// The LDS layouts (ptmcmc_amd/csrc/ptm_lds_layout.hpp) without a GPU.  Every layout is carved twice over the shapes below: by its own
// constructor, as the launch asks for `bytes`, and through a recording carve that notes each region as the layout takes it.  Checked for
// every shape: the two byte counts agree; every region lies inside `bytes`, is aligned to its element size (the first one to 16) and
// overlaps no other, except those the layout takes from a reuse() of earlier space, which must end inside that space; the layout's
// pointers over a heap buffer of exactly `bytes` can be written end to end (a sanitizer build sees every byte).  Decide's alias rule must
// flip inside the two pairs of ladders named below.  Prints {"rows": {shape: bytes}}: tests/test_lds_layout_cpu.py holds the table to
// tests/golden/lds_bytes.json.  (The lanes, fused and persistent ladder kernels are not built from a layout: no rows.)  Exit status 1 and a line per broken property on stderr.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "ptm_lds_layout.hpp"
#include "ptm_sweep_plan.hpp"

using namespace ptm;

static int failures = 0;
static std::map<std::string, size_t> table;   // (a shape met twice is one row)
static void broken(const std::string& row, const char* what, const char* region) {
  if (++failures <= 20) fprintf(stderr, "BROKEN: %s -- %s (%s)\n", what, row.c_str(), region);
}

static int strays = 0;   // pointers handed out that were not base + the offset noted for them

struct Region {
  const char* name;
  size_t off, len, elem, lim;   // lim: the end of the space a reusing region lives in (0: a region of its own)
  bool live;
};

// the recording carve: an LdsCarve that notes what is asked of it, and writes each live region through the pointer it hands out
struct Recorder {
  LdsCarve c;
  std::vector<Region>* out;
  size_t lim;
  const unsigned char* base;
  Recorder(void* b, std::vector<Region>* o) : c(b), out(o), lim(0), base(static_cast<unsigned char*>(b)) {}
  size_t at() const { return c.at(); }
  size_t size() const { return c.size(); }
  template <class T>
  void take(T*& p, const char* name, int n) {
    const size_t at = c.off;
    c.take(p, name, n);
    out->push_back({name, at, n * sizeof(T), sizeof(T), lim, c.live});
    if (reinterpret_cast<unsigned char*>(p) != base + at) ++strays;
    if (c.live && n) memset(p, 0x5a, n * sizeof(T));
  }
  void tail(bool on) { c.tail(on); }
  void slack(const char* name, size_t n) {
    if (c.live) out->push_back({name, c.bytes, n, 1, 0, true});
    c.slack(name, n);
  }
  template <class T>
  Recorder reuse(T* p, size_t begin, size_t end) const { Recorder r(*this); r.c = c.reuse(p, begin, end); r.lim = end; return r; }
};

// one shape of one layout: L is carved by carve(recorder, facts...) and by its constructor
template <class L, class... Facts>
static L layout_row(const std::string& row, Facts... facts) {
  const size_t bytes = L(nullptr, facts...).bytes;
  std::vector<Region> reg;
  void* buf = malloc(bytes);   // (16-byte aligned, as the kernels' LDS is)
  Recorder r(buf, &reg);
  L lay;
  lay.carve(r, facts...);
  free(buf);
  if (lay.bytes != bytes || r.c.bytes != bytes) broken(row, "the constructor and the recording carve disagree on bytes", "");
  if (strays) { broken(row, "a pointer is not where its offset says", ""); strays = 0; }
  if (reg.empty() || reg[0].off != 0) broken(row, "the first region starts the allocation", "");
  for (size_t i = 0; i < reg.size(); ++i) {
    const Region& a = reg[i];
    if (!a.live) continue;   // (a tail this shape does not have)
    if (a.off + a.len > bytes) broken(row, "a region ends past bytes", a.name);
    if (a.off % a.elem) broken(row, "a region is not aligned to its element", a.name);
    if (a.lim && a.off + a.len > a.lim) broken(row, "a reusing region ends past the space it reuses", a.name);
    for (size_t j = 0; j < i; ++j) {
      const Region& b = reg[j];
      if (!b.live || !a.len || !b.len || (a.lim != 0) != (b.lim != 0)) continue;   // (reusing regions may lie over regions of their own, not over each other)
      if (a.off < b.off + b.len && b.off < a.off + a.len) broken(row, "two regions overlap", a.name);
    }
  }
  table[row] = bytes;
  return lay;
}

static std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
static std::string fmt(const char* f, ...) {
  char b[256];
  va_list ap;
  va_start(ap, f);
  vsnprintf(b, sizeof b, f, ap);
  va_end(ap);
  return b;
}

static const int NTS[] = {2, 3, 5, 8, 71, 72, 300, 796, 800, 1024, 1100};
static const double RATES[] = {0.1, 0.3, 0.5};
static int ms_of(int Nt, double rate) { return (int)(1 + 2 * rate * Nt); }   // maxswapsperstep, as the engine sets it

template <int DP>
static void general_rows() {
  for (int uni = 0; uni < 2; ++uni)
    for (int kind : {PLAN_DENSE, PLAN_DIAG, PLAN_LOWER}) {
      const int stride = kind == PLAN_DIAG ? DP : DP * DP;   // the engine's prop_stride
      layout_row<GeneralLds>(fmt("general DP=%d uni=%d kind=%d stride=%d", DP, uni, kind, stride), uni && kind != PLAN_DIAG, stride);
    }
}

int main() {
  // decide: whole-ladder windows and two shard windows nloc + 1 + H (a half and an eighth of the ladder, H = 8); every legal tail
  const int tails[][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {1, 0, 1}, {1, 1, 1}};   // evolve, evb, cut
  std::map<std::string, bool> al;
  for (int Nt : NTS)
    for (double rate : RATES) {
      const int ms = ms_of(Nt, rate);
      for (int WN : {Nt, (Nt + 1) / 2 + 1 + 8, (Nt + 7) / 8 + 1 + 8}) {
        if (WN > Nt) WN = Nt;
        for (const auto& t : tails) {
          const DecideLds L = layout_row<DecideLds>(fmt("decide Nt=%d ms=%d WN=%d evolve=%d evb=%d cut=%d", Nt, ms, WN, t[0], t[1], t[2]), Nt, ms, WN, t[0] != 0, t[1] != 0, t[2] != 0);
          if (WN == Nt && t[0] && !t[1] && !t[2]) al[fmt("%d@%.1f", Nt, rate)] = L.aliased;
        }
      }
    }
  // both sides of the alias rule are among the rows
  if (al.at("71@0.5") == al.at("72@0.5")) broken("decide Nt=71 / 72 at swap rate 0.5", "the alias rule does not flip", "");
  if (al.at("796@0.1") == al.at("800@0.1")) broken("decide Nt=796 / 800 at swap rate 0.1", "the alias rule does not flip", "");
  for (int mgen = 0; mgen < 4; ++mgen)
    for (int cpt = 0; cpt < 2; ++cpt)
      for (int nrung : {1, 7, 564, 1024})
        layout_row<Mfma32Lds>(fmt("mfma32 mgen=%d compacted=%d nrung=%d", mgen, cpt, nrung), mgen != 0, cpt != 0, nrung);
  for (int nrung : {1, 7, 564, 1024}) {
    const size_t with = layout_row<BoxPreLds>(fmt("prepass nrung=%d", nrung), true, nrung).bytes;
    const size_t without = layout_row<BoxPreLds>(fmt("prepass tables=0 nrung=%d", nrung), false, nrung).bytes;
    if (with - without != BM_TABLE_DOUBLES * sizeof(double)) broken(fmt("prepass nrung=%d", nrung), "the table-free layout is not the tables smaller", "bm");
  }
  general_rows<4>(); general_rows<8>(); general_rows<16>(); general_rows<32>();
  layout_row<Mfma64Lds>("mfma64");
  layout_row<Mfma128Lds>("mfma128");

  printf("{\"rows\": {\n");
  size_t i = 0;
  for (const auto& kv : table) printf(" \"%s\": %zu%s\n", kv.first.c_str(), kv.second, ++i < table.size() ? "," : "");
  printf("}}\n");
  return failures ? 1 : 0;
}
