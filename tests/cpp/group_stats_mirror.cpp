// Drives pcgx::KDTree::GroupStats (pcgol_amd/host/pcgx.hpp) over the C ABI and prints what tests/test_cpp_group_stats.py
// compares with the Python binding's results.
// Input: a text file written by the test
//   P n      followed by n lines "x y z": the cloud (a tree over it)
//   C r      Clusters(r), then GroupStats of its result
// Output per C: "N count ..." (one per cluster), then one line per output array with every value as the hexadecimal
// bits of a float64 ("A" aabb widened, "M" centroid, "V" cov, "E" eig, "X" axes, "O" obb).
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../../pcgol_amd/host/pcgx.hpp"

template <class T>
static void bits(const char *tag, const std::vector<T> &v) {
  std::printf("%s", tag);
  for (T x : v) {
    const double d = (double)x;
    uint64_t b;
    std::memcpy(&b, &d, 8);
    std::printf(" %016" PRIx64, b);
  }
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  try {
    pcgx::check(pcgx_init(0));
    pcgx::CheckAbi();
    std::ifstream in(argv[1]);
    std::string tag;
    std::unique_ptr<pcgx::KDTree> tree;
    while (in >> tag) {
      if (tag == "P") {
        size_t n;
        in >> n;
        std::vector<pcgx::Vec3> pts(n);
        for (size_t i = 0; i < n; i++) in >> pts[i][0] >> pts[i][1] >> pts[i][2];
        tree.reset(new pcgx::KDTree(pts));
      } else if (tag == "C") {
        float r;
        in >> r;
        const auto g = tree->GroupStats(tree->Clusters(r));
        std::printf("N");
        for (int64_t x : g.count) std::printf(" %" PRId64, x);
        std::printf("\n");
        bits("A", g.aabb);
        bits("M", g.centroid);
        bits("V", g.cov);
        bits("E", g.eig);
        bits("X", g.axes);
        bits("O", g.obb);
      }
    }
  } catch (const pcgx::Error &e) {
    std::fprintf(stderr, "pcgx error %d: %s\n", (int)e.code, e.what());
    return 1;
  }
  return 0;
}
