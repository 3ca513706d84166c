// Drives pcgx::KDTree::CylinderStats and pcgx::M3C2Finish (pcgol_amd/host/pcgx.hpp) over the C ABI and prints what
// tests/test_cpp_m3c2.py compares with the Python binding's results.
// Input: a text file written by the test
//   P n        followed by n lines "x y z"                 an epoch's cloud (a tree over it); the first is epoch 1
//   C m        followed by m lines "ox oy oz dx dy dz"      the cores and axes
//   Q rho L e k   the statistics of both epochs at that radius and half length, and the finish with registration
//                 error e and minimum count k
// Output: per Q seven lines: "N1 count ...", "S1 sum ..." (hexadecimal floats), "N2 ...", "S2 ...", "D distance ...",
// "L lod ...", "G significant ...".
#include <cstdio>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../../pcgol_amd/host/pcgx.hpp"

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  try {
    pcgx::check(pcgx_init(0));
    pcgx::CheckAbi();
    std::ifstream in(argv[1]);
    std::string tag;
    std::vector<std::unique_ptr<pcgx::KDTree>> trees;
    std::vector<pcgx::Vec3> o, d;
    while (in >> tag) {
      if (tag == "P") {
        size_t n;
        in >> n;
        std::vector<pcgx::Vec3> pts(n);
        for (size_t i = 0; i < n; i++) in >> pts[i][0] >> pts[i][1] >> pts[i][2];
        trees.emplace_back(new pcgx::KDTree(pts));
      } else if (tag == "C") {
        size_t m;
        in >> m;
        o.assign(m, pcgx::Vec3{});
        d.assign(m, pcgx::Vec3{});
        for (size_t i = 0; i < m; i++) in >> o[i][0] >> o[i][1] >> o[i][2] >> d[i][0] >> d[i][1] >> d[i][2];
      } else if (tag == "Q") {
        float rho, half;
        double reg;
        int k;
        in >> rho >> half >> reg >> k;
        if (trees.size() != 2) return 2;
        const auto e1 = trees[0]->CylinderStats(o, d, rho, half);
        const auto e2 = trees[1]->CylinderStats(o, d, rho, half);
        const auto r = pcgx::M3C2Finish(d, e1, e2, reg, (int32_t)k);
        const pcgx::KDTree::CylinderStatsResult *es[2] = {&e1, &e2};
        for (int e = 0; e < 2; e++) {
          std::printf("N%d", e + 1);
          for (int32_t c : es[e]->counts) std::printf(" %d", (int)c);
          std::printf("\nS%d", e + 1);
          for (double s : es[e]->sums) std::printf(" %a", s);
          std::printf("\n");
        }
        std::printf("D");
        for (double v : r.distance) std::printf(" %a", v);
        std::printf("\nL");
        for (double v : r.lod) std::printf(" %a", v);
        std::printf("\nG");
        for (uint8_t v : r.significant) std::printf(" %d", (int)v);
        std::printf("\n");
      }
    }
  } catch (const pcgx::Error &e) {
    std::fprintf(stderr, "pcgx error %d: %s\n", (int)e.code, e.what());
    return 1;
  }
  return 0;
}
