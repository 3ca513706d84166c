// Drives pcgx::KDTree::KNearestBatch and pcgx::StatisticalOutlierRemoval (pcgol_amd/host/pcgx.hpp) over the C ABI and
// prints what tests/test_cpp_knearest.py compares with the Python binding's results.
// Input: a text file written by the test
//   P n              followed by n lines "x y z"   the cloud (a tree over it)
//   K k r m          followed by m lines "x y z"   KNearestBatch(queries, k, r); m == 0: the tree's own points
//   S meanK mul neg                                StatisticalOutlierRemoval(meanK, mul).WithNegative(neg) on the cloud
// Output: K: one line per query "count id dsq id dsq ..."; S: "kept mu sigma T" then one line per kept point "x y z"
// (%.9g: float32 round trips exactly; %.17g for float64).
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
    std::vector<pcgx::Vec3> pts;
    std::unique_ptr<pcgx::KDTree> tree;
    while (in >> tag) {
      if (tag == "P") {
        size_t n;
        in >> n;
        pts.resize(n);
        for (auto &p : pts) in >> p[0] >> p[1] >> p[2];
        tree.reset(new pcgx::KDTree(pts));
      } else if (tag == "K") {
        int32_t k;
        float r;
        size_t m;
        in >> k >> r >> m;
        std::vector<pcgx::Vec3> q(m);
        for (auto &p : q) in >> p[0] >> p[1] >> p[2];
        for (const auto &row : tree->KNearestBatch(q, k, r)) {
          std::printf("%d", (int)row.size());
          for (const auto &nb : row) std::printf(" %" PRId64 " %.9g", nb.ID, nb.DistSq);
          std::printf("\n");
        }
      } else if (tag == "S") {
        int32_t k, neg;
        float mul;
        in >> k >> mul >> neg;
        pcgx::StatisticalOutlierRemoval f(k, mul);
        f.WithNegative(neg != 0);
        const auto out = f.Filter(pcgx::CloudView{pts.data(), (int64_t)pts.size(), 12, 0});
        const size_t kept = out.size() / 12;
        std::printf("%zu %.17g %.17g %.17g\n", kept, f.Stats[0], f.Stats[1], f.Stats[2]);
        for (size_t i = 0; i < kept; i++) {
          float v[3];
          std::memcpy(v, out.data() + 12 * i, 12);
          std::printf("%.9g %.9g %.9g\n", v[0], v[1], v[2]);
        }
      }
    }
  } catch (const pcgx::Error &e) {
    std::fprintf(stderr, "pcgx error %d: %s\n", (int)e.code, e.what());
    return 1;
  }
  return 0;
}
