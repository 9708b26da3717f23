// The single-precision box pre-pass's margin (ptmcmc_amd/csrc/ptm_sweep_plan.hpp: prefilter_margins) without a GPU.  The kernel forms
// rows 0..15 of T z in float from normals that are off by up to PTM_BP_DZ each; the margin m_d must cover the distance between that
// and the double-precision product of the exact normals, for every factor and every order of summation -- then "outside by more than
// m_d" implies "outside".  Exit status 1 and a line per broken property on stderr.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "ptm_sweep_plan.hpp"

using namespace ptm;

static int failures = 0;
static void check(bool ok, const char* what) {
  if (!ok) { ++failures; fprintf(stderr, "BROKEN: %s\n", what); }
}

static const int D = 32, ND = PREFILTER_DIMS;
static const double ZMAX = 6.76;   // sqrt(-2 ln 2^-33) = 6.7637: the largest radius Box-Muller draws from 32 bits

// row d of T z in float, the terms taken in the order `ord`: plain multiply-and-add, fused, pairwise, or Kahan-free blocks of four
// summed apart (what four chained matrix instructions of depth four do when each starts from zero)
static float product_f32(const double* Trow, const float* z, const int* ord, int n, int how) {
  float t[ND], s = 0.0f;
  for (int k = 0; k < n; ++k) t[k] = (float)Trow[ord[k]];
  switch (how) {
    case 0: for (int k = 0; k < n; ++k) s = s + t[k] * z[ord[k]]; return s;
    case 1: for (int k = 0; k < n; ++k) s = std::fmaf(t[k], z[ord[k]], s); return s;
    case 2: {
      float p[ND];
      for (int k = 0; k < ND; ++k) p[k] = k < n ? t[k] * z[ord[k]] : 0.0f;
      for (int w = ND / 2; w >= 1; w /= 2) for (int k = 0; k < w; ++k) p[k] = p[k] + p[k + w];
      return p[0];
    }
    default: {
      float b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      for (int k = 0; k < n; ++k) b[k / 4] = std::fmaf(t[k], z[ord[k]], b[k / 4]);
      return (b[0] + b[1]) + (b[2] + b[3]);
    }
  }
}

int main() {
  std::mt19937_64 rng(20251);
  std::uniform_real_distribution<double> un(-1.0, 1.0);
  check(PTM_BP_DZ > 0.0 && PTM_BP_DZ < 1e-2 && PTM_BP_F32_SLACK > 0.0 && PTM_BP_F32_SLACK < PTM_BP_DZ, "the constants: a normal is good to a few digits, the product's rounding is the smaller term");
  check(prefilter_margin(0.0) == 0.0, "a zero row has no margin: its product is 0 in either precision");
  check(std::isinf(prefilter_margin(INFINITY)) && std::isinf(prefilter_margin(NAN)) && std::isinf(prefilter_margin(1e38)), "a row float cannot hold settles nothing");
  {   // monotone in |T|
    double prev = 0.0;
    bool mono = true;
    for (double s = 1e-300; s < 1e39; s *= 7.3) { const double m = prefilter_margin(s); mono = mono && m >= prev && m > 0.0; prev = m; }
    check(mono, "the margin grows with sum |T|");
  }

  // the factors: scale 1e-30 .. 1e30, lower-triangular and diagonal, some rows zero, some entries zero
  const double scales[] = {1e-30, 1e-12, 1e-3, 1.0, 37.5, 1e6, 1e18, 1e30};
  double worst = 0.0;   // the largest deviation seen, as a share of the margin
  for (double scale : scales)
    for (int diag = 0; diag < 2; ++diag)
      for (int rep = 0; rep < 6; ++rep) {
        std::vector<double> T((size_t)D * D, 0.0), sig(D, 0.0);
        for (int i = 0; i < D; ++i) {
          const bool zero_row = (rng() % 5) == 0;
          sig[i] = zero_row ? 0.0 : scale * un(rng);
          for (int k = 0; k <= i; ++k) T[(size_t)i * D + k] = (zero_row || (rng() % 4) == 0) ? 0.0 : scale * un(rng) * std::pow(10.0, 3.0 * un(rng));
        }
        double m[ND], m2[ND];
        prefilter_margins(diag != 0, diag ? sig.data() : T.data(), D, m);
        // |T| grown entry by entry: no margin shrinks
        {
          std::vector<double> Tb(T), sb(sig);
          for (double& v : Tb) v *= 1.0 + 0.5 * std::fabs(un(rng));
          for (double& v : sb) v *= 1.0 + 0.5 * std::fabs(un(rng));
          prefilter_margins(diag != 0, diag ? sb.data() : Tb.data(), D, m2);
          bool mono = true;
          for (int d = 0; d < ND; ++d) mono = mono && m2[d] >= m[d];
          check(mono, "prefilter_margins is monotone in |T|");
        }
        for (int d = 0; d < ND; ++d) {
          double row[ND] = {0.0}, sumabs = 0.0;
          for (int k = 0; k < ND; ++k) { row[k] = diag ? (k == d ? sig[d] : 0.0) : T[(size_t)d * D + k]; sumabs += std::fabs(row[k]); }
          if (sumabs == 0.0) check(m[d] == 0.0, "a zero row's margin is 0");
          else check(m[d] > 0.0 && std::isfinite(m[d]), "a row float can hold has a finite margin");
          for (int draw = 0; draw < 40; ++draw) {
            double z[ND];
            float zf[ND];
            for (int k = 0; k < ND; ++k) {
              // an exact normal anywhere in the range (every fourth at its end), the kernel's off by up to PTM_BP_DZ and then rounded to float
              z[k] = (draw % 4 == 0 ? (un(rng) < 0 ? -1.0 : 1.0) : un(rng)) * ZMAX;
              const double off = (draw % 2 == 0 ? (un(rng) < 0 ? -1.0 : 1.0) : un(rng)) * PTM_BP_DZ * (1.0 - 1e-7);   // (the float rounding of z is part of PTM_BP_DZ)
              zf[k] = (float)(z[k] + off);
              if (std::fabs((double)zf[k] - z[k]) > PTM_BP_DZ) zf[k] = (float)z[k];
            }
            double exact = 0.0;
            for (int k = 0; k < ND; ++k) exact = std::fma(row[k], z[k], exact);
            int ord[ND];
            for (int k = 0; k < ND; ++k) ord[k] = k;
            for (int o = 0; o < 3; ++o) {
              if (o == 1) std::reverse(ord, ord + ND);
              if (o == 2) std::shuffle(ord, ord + ND, rng);
              for (int how = 0; how < 4; ++how) {
                const double dev = std::fabs((double)product_f32(row, zf, ord, ND, how) - exact);
                if (!(dev <= m[d])) { check(false, "the float product strays from the exact one by more than the margin"); fprintf(stderr, "  scale %g diag %d row %d order %d sum %d: deviation %g, margin %g\n", scale, diag, d, o, how, dev, m[d]); }
                if (m[d] > 0.0) worst = std::max(worst, dev / m[d]);
              }
            }
          }
        }
      }
  check(worst > 0.3, "the draws reach a fair share of the margin: the test is not vacuous");
  if (failures) fprintf(stderr, "%d broken properties\n", failures);
  else printf("ok\n");
  return failures ? 1 : 0;
}
