// Drives pcgx::KDTree::RayCast and RayPierce (pcgol_amd/host/pcgx.hpp) over the C ABI and prints what
// tests/test_cpp_rays.py compares with the Python binding's results.
// Input: a text file written by the test
//   P n        followed by n lines "x y z"                       the cloud (a tree over it)
//   R m b      followed by m lines "ox oy oz dx dy dz [lo hi]"    the rays; b = 1: with s_min and s_max
//   Q rho      RayCast and RayPierce of the rays at that radius
// Output: per Q four lines: "I id ...", "A along ...", "O off_sq ..." (both as hexadecimal floats), "C count ...".
#include <cinttypes>
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
    std::unique_ptr<pcgx::KDTree> tree;
    std::vector<pcgx::Vec3> o, d;
    std::vector<float> lo, hi;
    while (in >> tag) {
      if (tag == "P") {
        size_t n;
        in >> n;
        std::vector<pcgx::Vec3> pts(n);
        for (size_t i = 0; i < n; i++) in >> pts[i][0] >> pts[i][1] >> pts[i][2];
        tree.reset(new pcgx::KDTree(pts));
      } else if (tag == "R") {
        size_t m;
        int bounded;
        in >> m >> bounded;
        o.assign(m, pcgx::Vec3{});
        d.assign(m, pcgx::Vec3{});
        lo.assign(bounded ? m : 0, 0.0f);
        hi.assign(bounded ? m : 0, 0.0f);
        for (size_t i = 0; i < m; i++) {
          in >> o[i][0] >> o[i][1] >> o[i][2] >> d[i][0] >> d[i][1] >> d[i][2];
          if (bounded) in >> lo[i] >> hi[i];
        }
      } else if (tag == "Q") {
        float rho;
        in >> rho;
        const auto hits = tree->RayCast(o, d, rho, lo, hi);
        const auto counts = tree->RayPierce(o, d, rho, lo, hi);
        std::printf("I");
        for (int64_t id : hits.ids) std::printf(" %" PRId64, id);
        std::printf("\nA");
        for (double a : hits.along) std::printf(" %a", a);
        std::printf("\nO");
        for (double c : hits.offSq) std::printf(" %a", c);
        std::printf("\nC");
        for (int32_t c : counts) std::printf(" %d", (int)c);
        std::printf("\n");
      }
    }
  } catch (const pcgx::Error &e) {
    std::fprintf(stderr, "pcgx error %d: %s\n", (int)e.code, e.what());
    return 1;
  }
  return 0;
}
