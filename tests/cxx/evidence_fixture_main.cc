// The facade's evidence_estimator and evidence_records on what tests/test_evidence_cpu.py sends (no GPU, no engine call).
// stdin, whitespace separated:
//   ladder Nt W add_every_N ilen   then per chain (rung-major, chain = rung * W + walker): Nhist nrows llike[0..nrows-1]
//                                  then beta[walker][rung] (W * Nt values: every walker's own ladder)
//   ladder_init Ninit Nt W add_every_N ilen ...   the same with the rows in the reference's raw numbering, Ninit initial rows in front
//   records n verbose v[0..n-1]
// stdout: per walker "w <evidence> | up.. | down.. | count.." (%.17g); per pushed value its lines, then "best <%.17g>".
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "ptmcmc_gpu.hh"

using namespace ptmgpu;

int main() {
  std::string what;
  while (std::cin >> what) {
    if (what == "ladder" || what == "ladder_init") {
      int Nt, W, a, ilen, Ninit = 1;
      if (what == "ladder_init") std::cin >> Ninit;
      std::cin >> Nt >> W >> a >> ilen;
      std::vector<long long> nhist((size_t)Nt * W);
      std::vector<std::vector<double> > rows((size_t)Nt * W);
      for (size_t c = 0; c < rows.size(); c++) {
        size_t n;
        std::cin >> nhist[c] >> n;
        rows[c].resize(n);
        for (size_t k = 0; k < n; k++) std::cin >> rows[c][k];
      }
      std::vector<double> beta((size_t)W * Nt);
      for (size_t k = 0; k < beta.size(); k++) std::cin >> beta[k];
      for (int w = 0; w < W; w++) {
        std::vector<long long> nh((size_t)Nt);
        for (int r = 0; r < Nt; r++) nh[(size_t)r] = nhist[(size_t)r * W + w];
        const evidence_estimator::result res = evidence_estimator::estimate(Nt, a, ilen, nh.data(), &beta[(size_t)w * Nt], [&](int rung, long long row, double& ll) {
          const std::vector<double>& v = rows[(size_t)rung * W + w];
          if (row < 0 || (size_t)row >= v.size()) return false;
          ll = v[(size_t)row];
          return true;
        }, Ninit);
        printf("w %.17g |", res.evidence);
        for (int i = 0; i < Nt - 1; i++) printf(" %.17g", res.up[(size_t)i]);
        printf(" |");
        for (int i = 0; i < Nt - 1; i++) printf(" %.17g", res.down[(size_t)i]);
        printf(" |");
        for (int r = 0; r < Nt; r++) printf(" %d", res.count[(size_t)r]);
        printf(" | %d\n", res.complete ? 1 : 0);
      }
    } else if (what == "records") {
      int n, verbose;
      std::cin >> n >> verbose;
      evidence_records rec;
      for (int k = 0; k < n; k++) {
        double v;
        std::cin >> v;
        fputs(rec.push(v, verbose != 0).c_str(), stdout);
        printf("best %.17g\n", rec.best());
      }
    } else {
      fprintf(stderr, "unknown block %s\n", what.c_str());
      return 2;
    }
  }
  return 0;
}
